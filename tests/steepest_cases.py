"""The problems and windows the PnormDescent / CoordinateDescent / NoSearch tests share (tests/test_ref_steepest.py licenses them on the CPU,
tests/test_gpu_steepest.py compares the GPU solvers QN_PNORM_DESCENT / QN_COORDINATE_DESCENT with the restatement tests/ref_steepest.py on them).

THE REFERENCE'S OWN TESTS (pnorm_descent.rs:91-193, coordinate_descent.rs:101-198): f = 1/2 (x0^2 + gamma x1^2), gamma = 90, from (180, 152), tol
1e-12, minimize(.., 1000, 100) with MoreThuente::default() and BackTracking::new(1e-4, 0.5); PnormDescent with inverse_p = diag(1, 1/gamma).
Asserted: |f| < 1e-6.  n = 2 is the literal-order path (n <= 5): these runs are compared decision for decision, exactly.

WINDOWS (PnormDescent beyond n = 5).  A window is a fixed number K of iterations of one problem with one line search and one inverse_p.  The sizes
are the smallest at which csrc/qn_pnorm.hip.h can go wrong: 7 (under one wave's width of 16-byte lanes), 130 (ragged rows and columns: n_pad =
144), 1030 (more than one workgroup's rows, more than one column step per lane), 4100 (just above the kernel's LDS column chunk of 4096).  Every
inverse_p beyond n = 2 is NOT symmetric: a positive diagonal plus a dense random perturbation.

ORDER SPREAD AND TOLERANCE -- the rule tests/broyden_cases.py states.  For every window the restatement is run in its two summation orders
(matvec = "dot" / "fsum"); the spread is the largest relative difference between the two over the x-trace, f, ||g||_inf and the steps t, each
relative to the compared array's largest magnitude.  The GPU's summation order is a third order beside those two, so

    tol = max(MARGIN * spread, FLOOR_ULP * 2^-52)        (relative to the compared magnitude)

with MARGIN = 8 and FLOOR_ULP = 16, both fixed before any GPU run; `spread` is the CPU measurement recorded beside each window, never a
measurement of the code under test (tests/test_ref_steepest.py re-measures it and fails when a recorded figure is exceeded).
"""
import numpy as np

import problems as P
import ref_steepest as R
import spg_cases as SC

TOL = 1e-12
KAPPA = 1e2
SPREAD_CAP = 1e-10
MARGIN = 8.0
FLOOR_ULP = 16.0
EPS = 2.0 ** -52
MAX_LS = 50
GAMMA = 90.0
X0_2D = np.array([180.0, 152.0])
LDS_CHUNK = 4096  # QN_PN_CH of csrc/qn_pnorm.hip.h


def two_var(gamma=GAMMA):
    """pnorm_descent.rs:99-103 / coordinate_descent.rs:109-113"""
    def fn(x):
        return 0.5 * (x[0] ** 2 + gamma * x[1] ** 2), np.array([x[0], gamma * x[1]])
    return fn


INVERSE_P_2D = np.array([[1.0, 0.0], [0.0, 1.0 / GAMMA]])  # DMatrix::from_iterator(2, 2, vec![1.0, 0.0, 0.0, 1.0 / gamma])

# the reference's four unit tests: (name, solver, line search, recorded iterations, recorded oracle calls) -- the counts are what the restatement
# gives (tests/test_ref_steepest.py re-derives them); the GPU runs must reproduce them exactly
REFERENCE_TESTS = (
    ("pnorm_morethuente", "pnorm", "mt", 1, 3),
    ("pnorm_backtracking", "pnorm", "bt", 1, 3),
    ("coordinate_descent_morethuente", "cd", "mt", 9, 37),
    ("coordinate_descent_backtracking", "cd", "bt", 332, 665),
)

# Windows: name -> dict(problem, n, ls, K, spread).  problem: "quad_host" (the seeded SPD quadratic of tests/problems.py through a host closure),
# "quad_dev" (the same matrix as a device objective), "chain" (examples/device_closure.hip, a device closure), "lse" (the log-sum-exp device
# objective).  spread: measured by tests/test_ref_steepest.py::test_window_is_licensed (printed there with -s), recorded here, rounded up.
WINDOWS = {}


def _w(name, problem, n, ls, K, spread):
    WINDOWS[name] = dict(problem=problem, n=n, ls=ls, K=K, spread=spread)


#   name          problem      n      ls    K   spread (CPU, two orders)
_w("p7_mt",       "quad_host", 7,     "mt", 6,  8.7e-17)
_w("p130_bt",     "quad_dev",  130,   "bt", 6,  5.4e-16)
_w("p1030_mt",    "chain",     1030,  "mt", 5,  3.3e-15)
_w("p4100_bt",    "lse",       4100,  "bt", 2,  1.3e-15)


# NoSearch with PnormDescent (tests/test_gpu_steepest.py::test_nosearch_gradient_descent_and_pnorm): the p7 problem, three full steps x + d
NOSEARCH_WINDOW = dict(problem="quad_host", n=7, ls="none", K=3, spread=8.7e-17)


def tolerance(w):
    """relative tolerance of a GPU comparison on window w (see the module docstring)"""
    return max(MARGIN * w["spread"], FLOOR_ULP * EPS)


def inverse_p(n, diag, seed=11):
    """a NON-symmetric inverse_p: the positive diagonal `diag` plus a dense perturbation a fiftieth of its smallest entry in row sum"""
    rng = np.random.default_rng(seed + n)
    e = rng.standard_normal((n, n)) * (0.02 * float(np.min(diag)) / n)
    return np.diag(diag) + e


def problem(w, qo):
    """-> dict(fn, x0, p, data): the host function of the window's problem, its start, inverse_p, what the device oracle is built from"""
    kind, n = w["problem"], w["n"]
    if kind in ("quad_host", "quad_dev"):
        diag = P.synth_diag(n, KAPPA)
        q = qo.synth_rows(n, 0, n, P.SEED, diag)
        b, x0 = P.synth_vectors(n, P.SEED)
        fn, data, pd = R.rs.quadratic_fn(q, b), (q, b), 1.0 / np.diag(q)
    elif kind == "chain":
        a, c, x0, _, _ = SC.chain_problem(n)
        fn, data, pd = SC.chain_fn(a, c), (a, c), np.full(n, 0.2)
    elif kind == "lse":
        a, c, mu, x0, _, _ = SC.lse_problem(96, n)
        fn, data, pd = SC.lse_fn(a, c, mu), (a, c, mu), np.full(n, 1.0)
    else:
        raise KeyError(kind)
    return dict(fn=fn, x0=np.asarray(x0, dtype=np.float64), p=inverse_p(n, pd), data=data)


def ref_line_search(ls, n, matvec="dot"):
    if ls == "mt":
        return R.MoreThuente(matvec)
    if ls == "bt":
        return R.BackTracking(1e-4, 0.5, n, matvec)
    if ls == "none":
        return R.NoSearch()
    raise KeyError(ls)


def run_ref(solver, fn, x0, ls, iters, p=None, matvec="dot", tol=TOL, max_ls=MAX_LS):
    """the restatement on one problem: (solver, oracle, status) with status "ok" / "max_iter" """
    o = R.MemoOracle(fn)
    n = len(x0)
    if solver == "pnorm":
        s = R.PnormDescent(tol, x0, p, matvec)
    elif solver == "cd":
        s = R.CoordinateDescent(tol, x0, matvec)
    else:
        s = R.GradientDescent(tol, x0, matvec)
    try:
        s.minimize(ref_line_search(ls, n, matvec), o, iters, max_ls)
        status = "ok"
    except R.MaxIterReached:
        status = "max_iter"
    return s, o, status


def rel_diff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.max(np.abs(b))), np.finfo(np.float64).tiny)
    return float(np.max(np.abs(a - b))) / scale


def run_summary(s):
    """what two runs of a window are compared on"""
    return dict(x=np.array(s.trace_x), f=np.array([r["f"] for r in s.trace]), gnorm=np.array([r["gnorm"] for r in s.trace]),
                t=np.array([r["t"] for r in s.trace]))


def spread_of(pr, w):
    base = run_summary(run_ref("pnorm", pr["fn"], pr["x0"], w["ls"], w["K"], pr["p"])[0])
    other = run_summary(run_ref("pnorm", pr["fn"], pr["x0"], w["ls"], w["K"], pr["p"], "fsum")[0])
    if other["x"].shape != base["x"].shape:
        return float("inf")
    return max(rel_diff(other[key], base[key]) for key in base)


_REF_CACHE = {}


def window_ref(name, qo):
    """the window's problem and its restatement run (reference order), computed once and shared by the tests that need it; callers do not modify it"""
    if name not in _REF_CACHE:
        w = WINDOWS[name]
        pr = problem(w, qo)
        _REF_CACHE[name] = (pr,) + run_ref("pnorm", pr["fn"], pr["x0"], w["ls"], w["K"], pr["p"])
    return _REF_CACHE[name]
