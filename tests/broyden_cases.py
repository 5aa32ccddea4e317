"""The problems and windows the Broyden tests share (tests/test_ref_broyden.py licenses the windows on the CPU, tests/test_gpu_broyden.py
compares the GPU solver QN_BROYDEN with the restatement tests/ref_broyden.py on them).

THE REFERENCE'S OWN TESTS (broyden.rs:135-234, broyden_b.rs:166-222): f = 1/2 ((x0 + 1)^2 + gamma (x1 - 1)^2), gamma = 1, from (180, 152), tol 1e-12,
run to convergence; asserted: f < 1e-6 (and has_converged).  With gamma = 1 the Hessian is the identity H starts from: the first step lands on the
minimum, a = s - H y = 0, and H never leaves I.  These runs check the call sequence and the convergence tests, not the update -- which is why the
WINDOWS below add a 2-D problem with gamma = 90 for the n <= 5 path.

WINDOWS.  A window is a fixed number K of iterations of one problem with one line search.  Broyden's update as the reference writes it is not
the textbook one and need not keep H positive definite; the windows stop while every value is finite, every step takes a real update, and
||H - H'||_max is clearly non-zero at the end (tests/test_ref_broyden.py asserts all three).

ORDER SPREAD.  For every window the restatement is run in its four floating-point orders (update literal / factored x mat-vec numpy.dot /
math.fsum); the spread is the largest relative difference to the reference's own order (literal, dot) over the x-trace, f, s_norm, y_norm and
the final H, each relative to the compared array's largest magnitude.  A window is licensed when its spread is below SPREAD_CAP.  The GPU's
summation order is a third order beside the two the spread samples, so the GPU tolerance of a window is

    tol = max(MARGIN * spread, FLOOR_ULP * 2^-52)        (relative to the compared magnitude)

with MARGIN = 8 and a floor of FLOOR_ULP = 16 ulp (the 2-D windows, whose four orders agree almost to the bit, would otherwise ask for
less than one rounding of a five-operation expression).  MARGIN and FLOOR_ULP were fixed before any GPU run; `spread` is the CPU measurement recorded
beside each window (tests/test_ref_broyden.py re-measures it and fails when a recorded figure is exceeded).
"""
import numpy as np

import problems as P
import ref_broyden as R
import spg_cases as SC

TOL = 1e-12
KAPPA = 1e2
SPREAD_CAP = 1e-10
MARGIN = 8.0
FLOOR_ULP = 16.0
EPS = 2.0 ** -52
MAX_LS = 50

UPDATES = ("literal", "factored")
MATVECS = ("dot", "fsum")


def two_var(gamma):
    def fn(x):
        return 0.5 * ((x[0] + 1.0) ** 2 + gamma * (x[1] - 1.0) ** 2), np.array([x[0] + 1.0, gamma * (x[1] - 1.0)])
    return fn


X0_2D = np.array([180.0, 152.0])
INF2 = np.array([np.inf, np.inf])

# the reference's own tests: (name, line search, bounded)
REFERENCE_TESTS = (("broyden_morethuente", "mt", False), ("broyden_backtracking", "bt", False), ("broyden_b_backtracking", "btb", True))

# Windows: name -> dict(problem, n, ls, box, K, spread).  problem: "two_var" (host closure, gamma = 90), "quad_host" (the seeded SPD quadratic of
# tests/problems.py through a host closure), "quad_dev" (the same matrix as a device objective), "chain" (examples/device_closure.hip), "lse"
# (the log-sum-exp device objective).  box: None, or the half-width of the solver's box (BroydenB; the bounded line searches get the same box).
# spread: measured by tests/test_ref_broyden.py::test_order_spread (printed there with -s), recorded here.
WINDOWS = {}


def _w(name, problem, n, ls, box, K, spread):
    WINDOWS[name] = dict(problem=problem, n=n, ls=ls, box=box, K=K, spread=spread)


#   name              problem      n     ls     box    K   spread (CPU, four orders; measured values rounded up)
_w("two_var_mt",      "two_var",   2,    "mt",  None,  4,  7.0e-18)
_w("two_var_bt",      "two_var",   2,    "bt",  None,  4,  1.8e-18)
_w("two_var_btb",     "two_var",   2,    "btb", 200.0, 2,  1.5e-15)
_w("q7_mt",           "quad_host", 7,    "mt",  None,  6,  8.3e-16)
_w("q7_bt",           "quad_host", 7,    "bt",  None,  6,  9.0e-16)
_w("q7_mtb",          "quad_host", 7,    "mtb", 0.5,   6,  8.9e-16)
_w("q130_mt",         "quad_dev",  130,  "mt",  None,  6,  8.5e-16)
_w("q130_btb",        "quad_dev",  130,  "btb", 0.5,   6,  1.1e-15)
_w("q384_bt",         "quad_dev",  384,  "bt",  None,  6,  7.5e-16)
_w("q384_mtb",        "quad_dev",  384,  "mtb", 0.5,   6,  5.8e-13)
_w("q1024_mt",        "quad_dev",  1024, "mt",  None,  5,  1.2e-15)
_w("chain200_mt",     "chain",     200,  "mt",  None,  6,  1.5e-15)
_w("lse64_mt",        "lse",       64,   "mt",  None,  6,  1.3e-15)

# the skip rule: the 2-D window problem in the box +-200 with BackTrackingB runs into s_norm < tol in its third iteration (step 8.9e-16):
# no update there, success at the next loop top
SKIP_CASE = dict(problem="two_var", n=2, ls="btb", box=200.0, K=10, spread=1.5e-15)


def tolerance(w):
    """relative tolerance of a GPU comparison on window w (see the module docstring)"""
    return max(MARGIN * w["spread"], FLOOR_ULP * EPS)


def problem(w, qo):
    """-> dict(fn, x0, lb, ub, data): the host function of the window's problem, its start, the solver's box (None: unbounded)"""
    kind, n = w["problem"], w["n"]
    if kind == "two_var":
        fn, x0, data = two_var(90.0), X0_2D.copy(), None
    elif kind in ("quad_host", "quad_dev"):
        diag = P.synth_diag(n, KAPPA)
        q = qo.synth_rows(n, 0, n, P.SEED, diag)
        b, x0 = P.synth_vectors(n, P.SEED)
        fn, data = R.rs.quadratic_fn(q, b), (q, b)
    elif kind == "chain":
        a, c, x0, _, _ = SC.chain_problem(n)
        fn, data = SC.chain_fn(a, c), (a, c)
    elif kind == "lse":
        a, c, mu, x0, _, _ = SC.lse_problem(96, n)
        fn, data = SC.lse_fn(a, c, mu), (a, c, mu)
    else:
        raise KeyError(kind)
    lb = ub = None
    if w["box"] is not None:
        lb, ub = np.full(n, -w["box"]), np.full(n, w["box"])
    return dict(fn=fn, x0=np.asarray(x0, dtype=np.float64), lb=lb, ub=ub, data=data)


def ref_line_search(ls, lb, ub, n):
    if ls == "mt":
        return R.MoreThuente()
    if ls == "bt":
        return R.BackTracking(1e-4, 0.5)
    if lb is None:
        lb, ub = np.full(n, -np.inf), np.full(n, np.inf)
    if ls == "mtb":
        return R.MoreThuenteB(lb, ub)
    return R.BackTrackingB(1e-4, 0.5, lb, ub)


def run_ref(pr, ls, iters, update="literal", matvec="dot", tol=TOL, max_ls=MAX_LS):
    """the restatement on one problem: (solver, oracle, status) with status "ok" / "max_iter" """
    o = R.MemoOracle(pr["fn"], projected_ls=(ls == "btb"))
    n = pr["x0"].size
    if pr["lb"] is None:
        s = R.Broyden(tol, pr["x0"], update, matvec)
    else:
        s = R.BroydenB(tol, pr["x0"], pr["lb"], pr["ub"], update, matvec)
    try:
        s.minimize(ref_line_search(ls, pr["lb"], pr["ub"], n), o, iters, max_ls)
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
    return dict(x=np.array(s.trace_x), f=np.array([r["f"] for r in s.trace]), s_norm=np.array([r["s_norm"] for r in s.trace]),
                y_norm=np.array([r["y_norm"] for r in s.trace]), h=s.h.copy())


def spread_of(pr, w):
    base = run_summary(run_ref(pr, w["ls"], w["K"])[0])
    worst = 0.0
    for u in UPDATES:
        for m in MATVECS:
            if (u, m) == ("literal", "dot"):
                continue
            other = run_summary(run_ref(pr, w["ls"], w["K"], u, m)[0])
            if other["x"].shape != base["x"].shape:
                return float("inf")
            for key in base:
                worst = max(worst, rel_diff(other[key], base[key]))
    return worst
