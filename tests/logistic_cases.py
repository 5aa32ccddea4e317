"""What tests/test_ref_logistic.py (CPU) and tests/test_gpu_logistic.py (GPU) share: the logistic-regression problems, the truths (computed once), and
the NewtonCG windows by newton_cg_cases' method and constants, unchanged.

PROBLEMS: a seeded Gaussian A (m x n), labels from a planted x* plus noise, mu = 0.5, x0 standard normal, weights drawn from {0, 0.5, 1, 3} (some rows
are masked), and the same with unit weights.  SHAPES are lse_hess_vec_cases.SHAPES: the smallest at which each KCH instance of logit_onepass_kernel and
each edge of the row cut can go wrong.

THE LICENCE of a window (newton_cg_cases): the case runs with numpy.dot, math.fsum and reversed dots, and twice more with every evaluation moved by up
to 8 ulp of f and 2 ulp of each g_i and every product moved by up to PRODUCT_UNITS = 4 units of 2^-53 on the scale A'(d o (|A| |v|)) + |mu| |v|; a
window ends at the first disagreement (x beyond LICENCE / ROUNDING_LICENCE, any decision) or at f's floor (lbfgs_cases.above_f_floor)."""
import functools
import zlib

import numpy as np

import cg_cases as C
import lbfgs_cases as L
import lse_hess_vec_cases as HV
import newton_cg_cases as NC
import ref_logistic as RL
import ref_newton_cg as RN
import ref_spg as R
import ref_wolfe as W

SHAPES = HV.SHAPES
SCALES = [1e-3, 1.0, 30.0]
MU = 0.5
SEED_BASE = 2000  # (problem (m, n) is seeded with SEED_BASE m + n; with this base every NewtonCG window below is licensed for the restatement ALONE --
                  # test_ref_logistic.py asserts it --; 1000, 4000, 5000 and 7000 leave (257, 200) a window of 2 to 5 where an interpolated step amplifies 2 ulp of g)
WEIGHT_VALUES = (0.0, 0.5, 1.0, 3.0)
TOO_WIDE = HV.TOO_WIDE
TOL, ITERS, MAX_LS = NC.TOL, NC.ITERS, NC.MAX_LS
MIN_WINDOW, LICENCE, ROUNDING_LICENCE, GPU_TOL, PRODUCT_UNITS = NC.MIN_WINDOW, NC.LICENCE, NC.ROUNDING_LICENCE, NC.GPU_TOL, NC.PRODUCT_UNITS
NEWTON_SHAPES = NC.SHAPES
SEARCHES = NC.SEARCHES
CASES = [(m, n, ls) for (m, n) in NEWTON_SHAPES for ls in SEARCHES]
CONVERGENCE = NC.CONVERGENCE
WOLFE = NC.WOLFE
NEG_MU = -40.0  # (3, 5): H = A' diag(d) A + mu I with d <= w / 4 -- g'Hg < 0 at x0 (asserted on the host by both test files), rule 4 at j = 0


def row_cut(m):
    """(G, per): the device's cut of the rows over workgroups -- workgroup b owns rows [b per, min(m, (b + 1) per))"""
    mrpr = 16 * ((m + 15) // 16)
    g = max(1, min(256, (mrpr + 3) // 4))
    return g, (mrpr + g - 1) // g


@functools.lru_cache(maxsize=None)
def problem(m, n, weighted=True):
    """(a, y, w, mu, x0, v), read-only, computed once"""
    rng = np.random.default_rng(SEED_BASE * m + n)
    a = rng.standard_normal((m, n))
    xs = rng.standard_normal(n) / np.sqrt(n)
    y = np.where(a @ xs + 0.5 * rng.standard_normal(m) >= 0.0, 1.0, -1.0)
    w = rng.choice(WEIGHT_VALUES, size=m) if weighted else np.ones(m)
    if weighted and m >= 3 and not np.any(w > 0.0):
        w[m // 2] = 1.0
    x0 = rng.standard_normal(n)
    v = rng.standard_normal(n)
    for arr in (a, y, w, x0, v):
        arr.setflags(write=False)
    return a, y, w, MU, x0, v


def masked_at_cut_edges(m, n):
    """problem(m, n) with the first and the last row of a workgroup's cut masked (workgroup 1 where there is one, and the last one that owns rows)"""
    a, y, w, mu, x0, v = problem(m, n)
    _, per = row_cut(m)
    w = w.copy()
    last_wg = (m - 1) // per
    for b in {min(1, last_wg), last_wg}:
        w[b * per] = 0.0
        w[min(m, (b + 1) * per) - 1] = 0.0
    w.setflags(write=False)
    return a, y, w, mu, x0, v


_truths = {}


def truth_at(m, n, scale, kind="weighted"):
    """(problem, x, truth_and_bound at x = scale x0 with the problem's v), computed once.  kind: weighted / unit / edges"""
    key = (m, n, scale, kind)
    if key not in _truths:
        pr = masked_at_cut_edges(m, n) if kind == "edges" else problem(m, n, kind == "weighted")
        a, y, w, mu, x0, v = pr
        x = scale * x0
        _truths[key] = (pr, x, RL.truth_and_bound(a, y, w, mu, x, v))
    return _truths[key]


def saturated_problem():
    """(a, y, w, mu, x, expected margins): a 4 x 3 problem whose margins z = y a'x are -800, +800, +800 (masked) and 0.5"""
    a = np.array([[800.0, 0.0, 0.0], [0.0, 800.0, 0.0], [0.0, 800.0, 0.0], [0.0, 0.0, 0.5]])
    y = np.array([-1.0, 1.0, 1.0, 1.0])
    w = np.array([1.0, 2.0, 0.0, 1.0])
    x = np.array([1.0, 1.0, 1.0])
    return a, y, w, MU, x, np.array([-800.0, 800.0, 800.0, 0.5])


# ---- NewtonCG: the restatement's runs and their windows ----
def line_search(kind, dot=np.dot):
    return NC.line_search(kind, dot)


def moved_product(a, y, w, mu, seed):
    """ref_logistic.logistic_hess_vec_at with every product moved by up to PRODUCT_UNITS units of 2^-53 on the scale A'(d o (|A| |v|)) + |mu| |v|"""
    plain = RL.logistic_hess_vec_at(a, y, w, mu)
    aa = np.abs(a)

    def at_x(x):
        hv = plain(x)
        d = RL.weights_f64(a, y, w, x)

        def moved(v):
            q = hv(v)
            av = np.abs(v)
            scale = aa.T @ (d * (aa @ av)) + abs(mu) * av
            rng = np.random.default_rng(zlib.crc32(np.ascontiguousarray(v).tobytes()) ^ seed)
            return q + PRODUCT_UNITS * 2.0 ** -53 * rng.uniform(-1.0, 1.0, q.size) * scale
        return moved
    return at_x


def run_ref(m, n, ls, iters=ITERS, order="numpy", seed=None, mu=None, tol=TOL, solver=None, max_inner=0):
    """The restatement (ref_newton_cg.NewtonCG on ref_logistic) on one case: (solver object, oracle, status)"""
    a, y, w, mu0, x0, _ = problem(m, n)
    mu = mu0 if mu is None else mu
    fn = RL.logistic_fn(a, y, w, mu)
    dot = C.DOTS[order]
    if seed is not None:
        fn, product = C.rounded_otherwise(fn, seed), moved_product(a, y, w, mu, seed)
    else:
        product = RL.logistic_hess_vec_at(a, y, w, mu)
    o = R.CountingOracle(fn)
    s = solver or RN.NewtonCG(tol, x0, product, max_inner=max_inner, dot=dot)
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


@functools.lru_cache(maxsize=None)
def licence(m, n, ls):
    """(window, worst disagreement between the summation orders inside it, length of the run) of one case"""
    a = ref_case(m, n, ls)[0]
    w, worst = NC.agreeing(a, [ref_case(m, n, ls, order)[0] for order in ("fsum", "reversed")], LICENCE)
    w = min(w, NC.agreeing(a, [ref_case(m, n, ls, "numpy", seed)[0] for seed in (1, 2)], ROUNDING_LICENCE)[0])
    return min(w, L.above_f_floor(a, ls)), worst, len(a.trace)


def window(m, n, ls):
    return licence(m, n, ls)[0]


# ---- the rest of the family: the existing restatements on logistic_fn, licensed the same way (three summation orders at LICENCE, two moved
# evaluations at ROUNDING_LICENCE, f's floor), at most FAMILY_WINDOW iterations ----
FAMILY_WINDOW = 12
FAMILY_TOL = 1e-10
FAMILY_BOX = 0.3
FAMILY_CASES = [("lbfgs", 96, 64), ("lbfgs", 5, 2050), ("cg", 96, 64), ("cg", 5, 2050), ("spg", 96, 64), ("plbfgs", 40, 65)]


def family_box(kind, n):
    if kind in ("spg", "plbfgs"):
        return np.full(n, -FAMILY_BOX), np.full(n, FAMILY_BOX)
    return np.full(n, -np.inf), np.full(n, np.inf)


def family_run(kind, m, n, iters=FAMILY_WINDOW, order="numpy", seed=None):
    """LBFGS(5) + StrongWolfe, NonlinearCG("pr+") + StrongWolfe(1e-4, 0.1), SpectralProjectedGradient + GLLQuadratic in a +-0.3 box, or
    ProjectedLBFGS(5) + BackTrackingB in that box, on ref_logistic.logistic_fn: (solver object, status)"""
    import ref_cg as RC
    import ref_lbfgs as RLB
    a, y, w, mu, x0, _ = problem(m, n)
    fn = RL.logistic_fn(a, y, w, mu)
    if seed is not None:
        fn = C.rounded_otherwise(fn, seed)
    dot = C.DOTS[order]
    o = R.CountingOracle(fn)
    lb, ub = family_box(kind, n)
    if kind == "lbfgs":
        s, ls = RLB.LBFGS(FAMILY_TOL, x0, lb, ub, m=5, dot=dot), W.StrongWolfe(dot=dot)
    elif kind == "cg":
        s, ls = RC.NonlinearCG(FAMILY_TOL, x0, variant="pr+", dot=dot), W.StrongWolfe(1e-4, 0.1, dot=dot)
    elif kind == "spg":
        s, ls = R.SpectralProjectedGradient(FAMILY_TOL, x0, o, lb, ub, dot=dot), R.GLLQuadratic(1e-4, 10, dot=dot)
    else:
        s, ls = RLB.LBFGS(FAMILY_TOL, x0, lb, ub, m=5, dot=dot), R.BackTrackingB(1e-4, 0.5, lb, ub, dot=dot)
    status = "ok"
    try:
        s.minimize(ls, o, iters, 50)
    except R.MaxIterReached:
        status = "max_iter"
    except W.NotDescent:
        status = "not_descent"
    return s, status


def _family_agreeing(a, others, within):
    w = min([len(a.trace)] + [len(o.trace) for o in others])
    for k in range(w):
        for o in others:
            same = a.trace[k]["n_evals"] == o.trace[k]["n_evals"] and a.trace[k]["ls_iters"] == o.trace[k]["ls_iters"]
            dx = float(np.linalg.norm(a.trace_x[k] - o.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k])))
            dt = abs(a.trace[k]["t"] - o.trace[k]["t"]) / abs(a.trace[k]["t"])
            if not same or not dx <= within or not dt <= within:
                return k
    return w


@functools.lru_cache(maxsize=None)
def family_licence(kind, m, n):
    """(the numpy.dot run, window) of one case of the rest of the family"""
    a = family_run(kind, m, n)[0]
    w = _family_agreeing(a, [family_run(kind, m, n, order=order)[0] for order in ("fsum", "reversed")], LICENCE)
    w = min(w, _family_agreeing(a, [family_run(kind, m, n, seed=seed)[0] for seed in (1, 2)], ROUNDING_LICENCE))
    return a, min(w, L.above_f_floor(a, "gll" if kind == "spg" else "bt"))


def neg_mu_curvature():
    """(g'Hg, g.g) at x0 of the (3, 5) problem with mu = NEG_MU, in float64: the host's check that rule 4 is met at j = 0"""
    a, y, w, _, x0, _ = problem(3, 5)
    g = RL.logistic_fn(a, y, w, NEG_MU)(x0)[1]
    return float(g @ RL.logistic_hess_vec_at(a, y, w, NEG_MU)(x0)(g)), float(g @ g)
