"""What tests/test_ref_multinomial.py (CPU) and tests/test_gpu_multinomial.py (GPU) share: the softmax-regression problems, the truths (computed once),
and the NewtonCG / family windows by newton_cg_cases' method and constants, unchanged.

PROBLEMS: a seeded Gaussian A (m x n), labels the argmax of a planted W plus Gumbel noise of scale 0.5, weights drawn from {0, 0.5, 1, 3} (some rows
are masked), mu = 0.5, x0 and v standard normal with N = K n entries (class-major); the seed is 2000 m + 31 n + K.

SHAPES (m, n, K), the smallest at which each thing in mnl_onepass_kernel can go wrong: (1, 1, 2) and (3, 1, 5) fewer rows than a tile and than
workgroups; (17, 7, 3) an odd class stride and a row-tile edge; (15 / 16 / 17, 8, 16) around the row padding; (64, 41, 17) one class past sixteen;
(33, 3, 64) two class groups of 32 classes a thread; (1031, 12, 4) per > 4 in the row cut, several tiles per workgroup; (20, 1024, 16) and (20, 256, 64)
N_pad = 16384 exactly (four and two waves per class group).

THE LICENCE of a window (newton_cg_cases): the case runs with numpy.dot, math.fsum and reversed dots, and twice more with every evaluation moved by up
to 8 ulp of f and 2 ulp of each g_i and every product moved by up to PRODUCT_UNITS = 4 units of 2^-53 on the scale of the product's bound; a window
ends at the first disagreement (x beyond LICENCE / ROUNDING_LICENCE, any decision) or at f's floor (lbfgs_cases.above_f_floor)."""
import functools
import zlib

import numpy as np

import cg_cases as C
import lbfgs_cases as L
import newton_cg_cases as NC
import ref_multinomial as RM
import ref_newton_cg as RN
import ref_spg as R
import ref_wolfe as W

SHAPES = [(1, 1, 2), (3, 1, 5), (17, 7, 3), (15, 8, 16), (16, 8, 16), (17, 8, 16), (64, 41, 17), (33, 3, 64), (1031, 12, 4), (20, 1024, 16), (20, 256, 64)]
# one shape per remaining instance of the kernel and per remaining cut of its threads (KC x NC, TJ), few rows each: 4x8, 8x8, 2x16, 4x16, 16x4, 32x2 at
# TJ = 512 or 256 -- the instances that spill registers among them --, and 32x1 at TJ = 64 (eight class groups of one wave, K = 200)
CUT_SHAPES = [(5, 2049, 4), (5, 2100, 7), (5, 8000, 2), (5, 4100, 3), (9, 963, 17), (5, 600, 27), (9, 60, 200)]
# K >= 128 with N_pad = 16384 exactly: W fills 128 KiB of LDS and the rows' scratch of a full tile of 8 rows would pass the workgroup's 160 KiB, so the
# plan halves the rows in use (RT = 4 of R = 8); the second shape has per = 5 rows in a workgroup's cut: two such tiles, the second one row long
LDS_SHAPES = [(9, 128, 128), (1031, 64, 256)]
SCALES = [1e-3, 1.0, 30.0]
MU = 0.5
SEED_BASE = 2000
WEIGHT_VALUES = (0.0, 0.5, 1.0, 3.0)
TOL, ITERS, MAX_LS = NC.TOL, NC.ITERS, NC.MAX_LS
MIN_WINDOW, LICENCE, ROUNDING_LICENCE, GPU_TOL, PRODUCT_UNITS = NC.MIN_WINDOW, NC.LICENCE, NC.ROUNDING_LICENCE, NC.GPU_TOL, NC.PRODUCT_UNITS
NEWTON_SHAPES = [(96, 16, 4), (40, 13, 5), (257, 40, 5), (64, 41, 17)]
DECISION_SHAPES = [(3, 1, 5)]  # (converges in a handful of iterations: decisions only, not MIN_WINDOW)
SEARCHES = NC.SEARCHES
CASES = [(m, n, k, ls) for (m, n, k) in NEWTON_SHAPES + DECISION_SHAPES for ls in SEARCHES]
WOLFE = NC.WOLFE
NEG_SHAPE = (3, 1, 5)
NEG_MU = -40.0  # H = sum_r a_r a_r' (x) w_r (diag(p_r) - p_r p_r') + mu I with the first part below w_r a_r^2 / 2: g'Hg < 0 at x0 (asserted on the host)


def row_cut(m):
    """(G, per): the device's cut of the rows over workgroups -- workgroup b owns rows [b per, min(m, (b + 1) per))"""
    mrpr = 16 * ((m + 15) // 16)
    g = max(1, min(256, (mrpr + 3) // 4))
    return g, (mrpr + g - 1) // g


@functools.lru_cache(maxsize=None)
def problem(m, n, k, weighted=True):
    """(a, y, w, k, mu, x0, v), read-only, computed once"""
    rng = np.random.default_rng(SEED_BASE * m + 31 * n + k)
    a = rng.standard_normal((m, n))
    wp = rng.standard_normal((k, n))
    y = np.argmax(a @ wp.T + 0.5 * rng.gumbel(size=(m, k)), axis=1).astype(np.int32)
    w = rng.choice(WEIGHT_VALUES, size=m) if weighted else np.ones(m)
    if weighted and m >= 3 and not np.any(w > 0.0):
        w[m // 2] = 1.0
    x0 = rng.standard_normal(k * n)
    v = rng.standard_normal(k * n)
    for arr in (a, y, w, x0, v):
        arr.setflags(write=False)
    return a, y, w, k, MU, x0, v


def variant(m, n, k, kind):
    """weighted / unit / edges (the first and the last row of a workgroup's cut masked) / absent (the last class carried by no row) /
    overflow (a masked row whose margins overflow from finite entries of A)"""
    if kind in ("weighted", "unit"):
        return problem(m, n, k, kind == "weighted")
    a, y, w, k, mu, x0, v = problem(m, n, k)
    a, y, w = a.copy(), y.copy(), w.copy()
    if kind == "edges":
        _, per = row_cut(m)
        last_wg = (m - 1) // per
        for b in {min(1, last_wg), last_wg}:
            w[b * per] = 0.0
            w[min(m, (b + 1) * per) - 1] = 0.0
    elif kind == "absent":
        y[y == k - 1] = 0
    elif kind == "overflow":
        r = m // 2
        a[r, :] = 1e300 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)  # finite entries; a_r . W_k overflows at overflow_point
        w[r] = 0.0
    for arr in (a, y, w):
        arr.setflags(write=False)
    return a, y, w, k, mu, x0, v


def overflow_point(pr):
    """x0 with the first column of every class at +-1e10: the masked row's margins are +-inf (their differences NaN), every other row's are of the
    order 1e10: saturated, finite"""
    x = pr[5].copy().reshape(pr[3], -1)
    x[:, 0] = 1e10 * np.where(np.arange(pr[3]) % 2 == 0, 1.0, -1.0)
    return x.ravel()


_truths = {}


def truth_at(m, n, k, scale, kind="weighted"):
    """(problem, x, truth_and_bound at x = scale x0 with the problem's v), computed once"""
    key = (m, n, k, scale, kind)
    if key not in _truths:
        pr = variant(m, n, k, kind)
        a, y, w, k, mu, x0, v = pr
        x = scale * x0
        _truths[key] = (pr, x, RM.truth_and_bound(a, y, w, k, mu, x, v))
    return _truths[key]


def saturated_problem():
    """(a, y, w, k, mu, x, spread): 4 rows, 3 classes, margins spread by 1600: row 0 labelled with the loser (loss = 1600), row 1 with the winner
    (loss 0), row 2 masked, row 3 mild"""
    a = np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.0, 0.5]])
    x = np.array([[800.0, 1.0], [-800.0, -1.0], [-800.0, 0.25]]).ravel()
    y = np.array([1, 0, 2, 1], dtype=np.int32)
    w = np.array([1.0, 2.0, 0.0, 1.0])
    return a, y, w, 3, MU, x, 1600.0


# ---- NewtonCG: the restatement's runs and their windows ----
def line_search(kind, dot=np.dot):
    return NC.line_search(kind, dot)


def moved_product(a, y, w, k, mu, seed):
    """ref_multinomial.multinomial_hess_vec_at with every product moved by up to PRODUCT_UNITS units of 2^-53 on the scale
    sum_r |a_rj| w_r p_rk (|u|_rk + sum_l p_rl |u|_rl) + |mu| |v|, |u| = |A| |V|'"""
    plain = RM.multinomial_hess_vec_at(a, y, w, k, mu)
    aa = np.abs(a)
    n = a.shape[1]
    wv = np.ones(a.shape[0]) if w is None else np.asarray(w, dtype=np.float64)

    def at_x(x):
        hv = plain(x)
        p = RM.probabilities_f64(a, y, w, k, x)

        def moved(v):
            q = hv(v)
            au = aa @ np.abs(v).reshape(k, n).T
            scale = ((wv[:, None] * p * (au + np.sum(p * au, axis=1)[:, None])).T @ aa).ravel() + abs(mu) * np.abs(v)
            rng = np.random.default_rng(zlib.crc32(np.ascontiguousarray(v).tobytes()) ^ seed)
            return q + PRODUCT_UNITS * 2.0 ** -53 * rng.uniform(-1.0, 1.0, q.size) * scale
        return moved
    return at_x


def run_ref(m, n, k, ls, iters=ITERS, order="numpy", seed=None, mu=None, tol=TOL, solver=None, max_inner=0):
    """The restatement (the unmodified ref_newton_cg.NewtonCG on ref_multinomial) on one case: (solver object, oracle, status)"""
    a, y, w, k, mu0, x0, _ = problem(m, n, k)
    mu = mu0 if mu is None else mu
    fn = RM.multinomial_fn(a, y, w, k, mu)
    dot = C.DOTS[order]
    if seed is not None:
        fn, product = C.rounded_otherwise(fn, seed), moved_product(a, y, w, k, mu, seed)
    else:
        product = RM.multinomial_hess_vec_at(a, y, w, k, mu)
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
def ref_case(m, n, k, ls, order="numpy", seed=None):
    return run_ref(m, n, k, ls, order=order, seed=seed)


@functools.lru_cache(maxsize=None)
def licence(m, n, k, ls):
    """(window, worst disagreement between the summation orders inside it, length of the run) of one case"""
    a = ref_case(m, n, k, ls)[0]
    w, worst = NC.agreeing(a, [ref_case(m, n, k, ls, order)[0] for order in ("fsum", "reversed")], LICENCE)
    w = min(w, NC.agreeing(a, [ref_case(m, n, k, ls, "numpy", seed)[0] for seed in (1, 2)], ROUNDING_LICENCE)[0])
    return min(w, L.above_f_floor(a, ls)), worst, len(a.trace)


def window(m, n, k, ls):
    return licence(m, n, k, ls)[0]


# ---- the rest of the family: the existing restatements on multinomial_fn, licensed the same way, at most FAMILY_WINDOW iterations ----
FAMILY_WINDOW = 12
FAMILY_TOL = 1e-10
FAMILY_BOX = 0.3
FAMILY_CASES = [("lbfgs", 96, 16, 4), ("cg", 96, 16, 4), ("spg", 96, 16, 4), ("plbfgs", 40, 13, 5)]


def family_box(kind, nn):
    if kind in ("spg", "plbfgs"):
        return np.full(nn, -FAMILY_BOX), np.full(nn, FAMILY_BOX)
    return np.full(nn, -np.inf), np.full(nn, np.inf)


def family_run(kind, m, n, k, iters=FAMILY_WINDOW, order="numpy", seed=None):
    """LBFGS(5) + StrongWolfe, NonlinearCG("pr+") + StrongWolfe(1e-4, 0.1), SpectralProjectedGradient + GLLQuadratic in a +-0.3 box, or
    ProjectedLBFGS(5) + BackTrackingB in that box, on ref_multinomial.multinomial_fn: (solver object, status)"""
    import ref_cg as RC
    import ref_lbfgs as RLB
    a, y, w, k, mu, x0, _ = problem(m, n, k)
    fn = RM.multinomial_fn(a, y, w, k, mu)
    if seed is not None:
        fn = C.rounded_otherwise(fn, seed)
    dot = C.DOTS[order]
    o = R.CountingOracle(fn)
    lb, ub = family_box(kind, k * n)
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
    for i in range(w):
        for o in others:
            same = a.trace[i]["n_evals"] == o.trace[i]["n_evals"] and a.trace[i]["ls_iters"] == o.trace[i]["ls_iters"]
            dx = float(np.linalg.norm(a.trace_x[i] - o.trace_x[i]) / max(1.0, np.linalg.norm(a.trace_x[i])))
            dt = abs(a.trace[i]["t"] - o.trace[i]["t"]) / abs(a.trace[i]["t"])
            if not same or not dx <= within or not dt <= within:
                return i
    return w


@functools.lru_cache(maxsize=None)
def family_licence(kind, m, n, k):
    """(the numpy.dot run, window) of one case of the rest of the family"""
    a = family_run(kind, m, n, k)[0]
    w = _family_agreeing(a, [family_run(kind, m, n, k, order=order)[0] for order in ("fsum", "reversed")], LICENCE)
    w = min(w, _family_agreeing(a, [family_run(kind, m, n, k, seed=seed)[0] for seed in (1, 2)], ROUNDING_LICENCE))
    return a, min(w, L.above_f_floor(a, "gll" if kind == "spg" else "bt"))


def neg_mu_curvature():
    """(g'Hg, g.g) at x0 of the NEG_SHAPE problem with mu = NEG_MU, in float64: the host's check that rule 4 is met at j = 0"""
    a, y, w, k, _, x0, _ = problem(*NEG_SHAPE)
    g = RM.multinomial_fn(a, y, w, k, NEG_MU)(x0)[1]
    return float(g @ RM.multinomial_hess_vec_at(a, y, w, k, NEG_MU)(x0)(g)), float(g @ g)
