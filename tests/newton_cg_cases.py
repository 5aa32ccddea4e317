"""The problems the NewtonCG tests share (tests/test_ref_newton_cg.py licenses the windows, tests/test_gpu_newton_cg.py uses them): the log-sum-exp
problems of spg_cases.lse_problem(m, n) from x0, BackTracking(1e-4, 0.5) and StrongWolfe(1e-4, 0.9), tol 1e-7 on ||g||_inf (at 1e-10 the runs stall
at f's last bit under Armijo: DESIGN.md 23-25), at most 40 iterations.  Every restatement run is made once and kept.

THE LICENCE of a window (the method of tests/test_ref_cg.py): the case runs with numpy.dot, with math.fsum of the products and with every dot
product summed in reversed order; and twice more with every evaluation moved pseudo-randomly by up to 8 ulp of f and 2 ulp of each g_i
(cg_cases.rounded_otherwise) AND every product H v moved by up to 4 units of 2^-53 (S |v|)_j -- the scale of tests/lse_hess_vec_cases.py's bound;
the device's products measure 0.00 to 0.66 of that unit against extended precision (tests/test_gpu_lse_hess_vec.py prints them), so this is at
least four times the device's own roundings.  A window ends at the first iteration where x differs by more than 1e-11 max(1, ||x||) between the
summation orders (2.5e-10 for the moved runs: a quarter of the 1e-9 the GPU tests allow), or where any decision differs -- t, n_evals, the inner
count j_k, an exit reason --, or where f's decrease falls below lbfgs_cases.above_f_floor's 1e4 ulp.  Windows are at least MIN_WINDOW iterations
or the whole run."""
import functools
import zlib

import numpy as np

import cg_cases as C
import lbfgs_cases as L
import ref_newton_cg as RN
import ref_spg as R
import ref_wolfe as W
import spg_cases as S

TOL = 1e-7
ITERS, MAX_LS = 40, 30
MIN_WINDOW = 6
LICENCE, ROUNDING_LICENCE = 1e-11, 2.5e-10
GPU_TOL = 1e-9
SHAPES = [(3, 5), (96, 64), (40, 65), (257, 200), (5, 2050)]
SEARCHES = ("bt", "wolfe")
CASES = [(m, n, ls) for (m, n) in SHAPES for ls in SEARCHES]
CONVERGENCE = [(96, 64), (40, 65), (257, 200)]  # BackTracking(1e-4, 0.5) from x0 to ||g||_inf < 1e-7
WOLFE = (1e-4, 0.9)
PRODUCT_UNITS = 4.0
NEG_MU = -1.0  # (3, 5) with this mu: g'Hg = -0.55 g.g at x0, rule 4 at j = 0 (checked on the host; with mu = -0.5 the first product is still positive,
               # 0.05 g.g, and rule 4 is met at j = 1)


@functools.lru_cache(maxsize=None)
def problem(m, n):
    a, c, mu, x0, _, _ = S.lse_problem(m, n)
    for v in (a, c, x0):
        v.setflags(write=False)
    return a, c, mu, x0


def line_search(kind, dot=np.dot):
    if kind == "wolfe":
        return W.StrongWolfe(WOLFE[0], WOLFE[1], dot=dot)
    return R.BackTracking(1e-4, 0.5, dot=dot)


def moved_product(a, c, mu, seed):
    """ref_newton_cg.lse_hess_vec_at with every product moved by up to PRODUCT_UNITS units of 2^-53 (S |v|)_j, seeded by the vector"""
    plain = RN.lse_hess_vec_at(a, c, mu)
    aa = np.abs(a)

    def at_x(x):
        hv = plain(x)
        z = a @ x + c
        e = np.exp(z - z.max())
        p = e / e.sum()
        g_abs = aa.T @ p

        def moved(v):
            q = hv(v)
            av = np.abs(v)
            scale = aa.T @ (p * (aa @ av)) + g_abs * float(g_abs @ av) + abs(mu) * av
            rng = np.random.default_rng(zlib.crc32(np.ascontiguousarray(v).tobytes()) ^ seed)
            return q + PRODUCT_UNITS * 2.0 ** -53 * rng.uniform(-1.0, 1.0, q.size) * scale
        return moved
    return at_x


def run_ref(m, n, ls, iters=ITERS, order="numpy", seed=None, eta_max=0.5, max_inner=0, mu=None, tol=TOL, solver=None):
    """The restatement on one case: (solver object, oracle, status).  seed: the moved evaluations and products; solver: continue that one."""
    a, c, mu0, x0 = problem(m, n)
    mu = mu0 if mu is None else mu
    fn = S.lse_fn(a, c, mu)
    dot = C.DOTS[order]
    if seed is not None:
        fn, product = C.rounded_otherwise(fn, seed), moved_product(a, c, mu, seed)
    else:
        product = RN.lse_hess_vec_at(a, c, mu)
    o = R.CountingOracle(fn)
    s = solver or RN.NewtonCG(tol, x0, product, eta_max=eta_max, max_inner=max_inner, dot=dot)
    status = "ok"
    try:
        s.minimize(line_search(ls, dot), o, iters, MAX_LS)
    except R.MaxIterReached:
        status = "max_iter"
    except W.NotDescent:
        status = "not_descent"
    return s, o, status


@functools.lru_cache(maxsize=None)
def ref_case(m, n, ls, order="numpy", seed=None):
    return run_ref(m, n, ls, order=order, seed=seed)


def agreeing(a, others, within):
    """(iterations at the front on which the runs agree, the worst relative difference in x and t inside them)"""
    w, worst = len(a.trace), 0.0
    for o in others:
        w = min(w, len(o.trace))
    for k in range(w):
        here = 0.0
        for o in others:
            same = (a.trace[k]["n_evals"] == o.trace[k]["n_evals"] and a.trace[k]["ls_iters"] == o.trace[k]["ls_iters"]
                    and a.inner[k] == o.inner[k] and a.why[k] == o.why[k])
            dx = float(np.linalg.norm(a.trace_x[k] - o.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k])))
            dt = abs(a.trace[k]["t"] - o.trace[k]["t"]) / abs(a.trace[k]["t"])
            if not same or not dx <= within or not dt <= within:
                return k, worst
            here = max(here, dx, dt)
        worst = max(worst, here)
    return w, worst


@functools.lru_cache(maxsize=None)
def licence(m, n, ls):
    """(window, worst disagreement between the summation orders inside it, length of the run) of one case"""
    a = ref_case(m, n, ls)[0]
    w, worst = agreeing(a, [ref_case(m, n, ls, order)[0] for order in ("fsum", "reversed")], LICENCE)
    w = min(w, agreeing(a, [ref_case(m, n, ls, "numpy", seed)[0] for seed in (1, 2)], ROUNDING_LICENCE)[0])
    return min(w, L.above_f_floor(a, ls)), worst, len(a.trace)


def window(m, n, ls):
    return licence(m, n, ls)[0]
