"""What tests/test_ref_precond.py (CPU) and tests/test_gpu_precond.py (GPU) share: the badly scaled logistic-regression problems NewtonCG's Jacobi
preconditioner is for, the restatement's runs with and without it (tests/ref_newton_pcg.py), and their windows by newton_cg_cases' method and
constants, unchanged.

PROBLEMS: a seeded Gaussian A (m x n) whose column j is scaled by 10^U(-SPREAD, SPREAD), labels from a planted x* on the columns brought to unit
size plus noise, unit weights, mu = 1e-3, x0 = 0.  kind "dense": qn.Logistic; kind "sparse": the same draw under sparse_logistic_cases' Bernoulli
pattern (density 0.25), qn.SparseLogistic.  SHAPES are (96, 64) and (257, 200); COUNTER is (40, 65), m < n with a small mu, where Jacobi is NOT better
(recorded, asserted on the CPU).  SEED_BASE: problem (m, n) is seeded with SEED_BASE m + n; chosen as logistic_cases.SEED_BASE was, so that every
window below is at least MIN_WINDOW or the whole run (test_ref_precond.py asserts it and lists what was tried).

THE LICENCE of a window (newton_cg_cases): the case runs with numpy.dot, math.fsum and reversed dots; and twice more with every evaluation moved by
up to 8 ulp of f and 2 ulp of each g_i, every product moved by PRODUCT_UNITS units of 2^-53 on its scale, and every diagonal moved by up to DIAG_UNITS
units of its derived bound (ref_newton_pcg.logistic_diag_truth).  A window ends at the first disagreement (x beyond LICENCE / ROUNDING_LICENCE, any
decision: t, n_evals, the inner count, the exit reason) or at f's floor."""
import functools
import zlib

import numpy as np

import cg_cases as C
import lbfgs_cases as L
import newton_cg_cases as NC
import ref_logistic as RL
import ref_newton_cg as RN
import ref_newton_pcg as RP
import ref_spg as R
import ref_wolfe as W
import sparse_logistic_cases as SL

SHAPES = [(96, 64), (257, 200)]
COUNTER = (40, 65)
KINDS = ("dense", "sparse")
SPREAD = 1.5
MU = 1e-3
SEED_BASE = 7
TOL, MAX_LS = NC.TOL, NC.MAX_LS
ITERS = 60  # (the plain runs need 36 to 41 outer iterations on these problems; newton_cg_cases' 40 would cut them short)
MIN_WINDOW, LICENCE, ROUNDING_LICENCE, GPU_TOL, PRODUCT_UNITS = NC.MIN_WINDOW, NC.LICENCE, NC.ROUNDING_LICENCE, NC.GPU_TOL, NC.PRODUCT_UNITS
DIAG_UNITS = 2.0
SEARCHES = NC.SEARCHES
WOLFE = NC.WOLFE
CASES = [(kind, m, n, ls) for kind in KINDS for (m, n) in SHAPES for ls in SEARCHES]
HALF = 0.5  # the condition: Jacobi's inner total is at most half the plain run's on SHAPES


@functools.lru_cache(maxsize=None)
def problem(m, n, kind="dense"):
    """dict(a (dense), y, w, mu, x0, scales; sparse: indptr, indices, data, mask), read-only, computed once"""
    rng = np.random.default_rng(SEED_BASE * m + n)
    a = rng.standard_normal((m, n))
    scales = 10.0 ** rng.uniform(-SPREAD, SPREAD, n)
    a = a * scales
    xs = rng.standard_normal(n) / np.sqrt(n)
    noise = 0.3 * rng.standard_normal(m)
    out = dict(mu=MU, x0=np.zeros(n), w=np.ones(m), scales=scales)
    if kind == "sparse":
        mask = SL._pattern(np.random.default_rng(SEED_BASE * m + n + 1), m, n, "weighted")
        a = np.where(mask, a, 0.0)
        indptr, indices, data = SL.to_csr(a, mask)
        out.update(indptr=indptr, indices=indices, data=data, mask=mask)
    colmax = np.abs(a).max(axis=0)
    out["y"] = np.where((a / np.where(colmax > 0.0, colmax, 1.0)) @ xs + noise >= 0.0, 1.0, -1.0)
    out["a"] = a
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _functions(pr, kind, order):
    """(fn, product, diag_at) with every inner product in the given summation order"""
    a, y, w, mu = pr["a"], pr["y"], pr["w"], pr["mu"]
    if kind == "sparse":
        fn, product = SL._ordered(pr, mu, order)
    elif order == "numpy":
        fn, product = RL.logistic_fn(a, y, w, mu), RL.logistic_hess_vec_at(a, y, w, mu)
    else:
        fn, product = RL.logistic_fn(a, y, w, mu, C.DOTS[order]), RL.logistic_hess_vec_at(a, y, w, mu, C.DOTS[order])
    return fn, product, RP.logistic_diag_at(a, y, w, mu, None if order == "numpy" else C.DOTS[order])


def moved_diag(pr, seed):
    """ref_newton_pcg.logistic_diag_at with every entry moved by up to DIAG_UNITS units of its derived bound, seeded by the point"""
    a, y, w, mu = pr["a"], pr["y"], pr["w"], pr["mu"]
    plain = RP.logistic_diag_at(a, y, w, mu)

    def at_x(x):
        bound = RP.logistic_diag_truth(a, y, w, mu, x)[1].astype(np.float64)
        rng = np.random.default_rng(zlib.crc32(np.ascontiguousarray(x).tobytes()) ^ seed ^ 0x5EED)
        return plain(x) + DIAG_UNITS * rng.uniform(-1.0, 1.0, x.size) * bound
    return at_x


def line_search(ls, dot=np.dot):
    return NC.line_search(ls, dot)


def run_ref(kind, m, n, ls, precond="jacobi", iters=ITERS, order="numpy", seed=None, solver=None, twice=False):
    """The restatement on one case: (solver object, oracle, status).  seed: the moved evaluations, products and diagonals"""
    pr = problem(m, n, kind)
    fn, product, diag_at = _functions(pr, kind, order)
    if seed is not None:
        fn = C.rounded_otherwise(fn, seed)
        product = SL.moved_product(pr, pr["mu"], seed)
        diag_at = moved_diag(pr, seed)
    dot = C.DOTS[order]
    o = R.CountingOracle(fn)
    if solver is None:
        solver = (RP.JacobiNewtonCG(TOL, pr["x0"], product, diag_at, dot=dot, twice=twice) if precond == "jacobi"
                  else RN.NewtonCG(TOL, pr["x0"], product, dot=dot))
    status = "ok"
    try:
        solver.minimize(line_search(ls, dot), o, iters, MAX_LS)
    except R.MaxIterReached:
        status = "max_iter"
    except W.NotDescent:
        status = "not_descent"
    return solver, o, status


@functools.lru_cache(maxsize=None)
def ref_case(kind, m, n, ls, precond="jacobi", order="numpy", seed=None):
    return run_ref(kind, m, n, ls, precond, order=order, seed=seed)


@functools.lru_cache(maxsize=None)
def licence(kind, m, n, ls):
    """(window, worst disagreement between the summation orders inside it, length of the run) of one preconditioned case"""
    a = ref_case(kind, m, n, ls)[0]
    w, worst = NC.agreeing(a, [ref_case(kind, m, n, ls, "jacobi", order)[0] for order in ("fsum", "reversed")], LICENCE)
    w = min(w, NC.agreeing(a, [ref_case(kind, m, n, ls, "jacobi", "numpy", seed)[0] for seed in (1, 2)], ROUNDING_LICENCE)[0])
    return min(w, L.above_f_floor(a, ls)), worst, len(a.trace)


def window(kind, m, n, ls):
    return licence(kind, m, n, ls)[0]


def final_gnorm(kind, m, n, solver):
    pr = problem(m, n, kind)
    return float(np.max(np.abs(RL.logistic_fn(pr["a"], pr["y"], pr["w"], pr["mu"])(solver.x)[1])))
