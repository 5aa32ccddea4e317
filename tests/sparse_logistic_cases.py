"""What tests/test_ref_sparse_logistic.py (CPU) and tests/test_gpu_sparse_logistic.py (GPU) share: the sparse logistic-regression problems, the truths
(computed once), the device's static cut restated from its documented rule, and the NewtonCG / family windows by logistic_cases' method and constants.

PROBLEMS: a seeded Bernoulli pattern with Gaussian values (m x n, CSR with sorted columns), labels from a planted x* plus noise, mu = 0.5, x0 and v
standard normal, weights drawn from {0, 0.5, 1, 3}.  THE TRUTH is ref_logistic.truth_and_bound on the DENSIFIED matrix: its bounds hold for any
summation order and any row length up to n (an absent entry is an exact zero: it adds nothing to zeta_r or to any other term of a bound), and they are
derived, not measured.  The criterion is |error| / bound <= 1 for f, g, d, q and v'Hv.

SHAPES, the smallest at which each part can go wrong:
    (1, 1), (3, 5)        fewer rows than one trip
    (40, 65)              row lengths 0 .. 64 drawn from the first 64 columns: an empty row (margin 0, loss w log 2) and an empty column, the last
                          (g_j = mu x_j); run with every L forced on both passes.  Kind "full" is the same shape with row lengths 0 .. 65 (a full
                          row then leaves no column empty, so the two are two problems)
    (96, 64)              density 0.25: automatic lanes
    (5, 2050)             one full row (2050 > SPQ_LONG_ROW = 2048 entries): the long-row path of the row pass
    (2050, 7)             a column of ones and two more entries per row: the long-row path of the column pass, 3 workgroups in the row cut
    (4096, 300)           density 0.9: more than 256 workgroups in both cuts (the strided fold; NewtonCG's kcount = 1)
    (64, 20000)           8 per row: n_pad beyond the dense Logistic's 16384
    (257, 200)            density 0.25: NewtonCG's convergence shape (not in SHAPES)

THE LICENCE of a window is logistic_cases' (newton_cg_cases' method and constants, unchanged): three summation orders at LICENCE, two runs with moved
evaluations and products at ROUNDING_LICENCE, f's floor."""
import functools
import zlib

import numpy as np

import cg_cases as C
import lbfgs_cases as L
import logistic_cases as LC
import newton_cg_cases as NC
import ref_logistic as RL
import ref_newton_cg as RN
import ref_spg as R
import ref_wolfe as W

SHAPES = [(1, 1), (3, 5), (40, 65), (96, 64), (5, 2050), (2050, 7), (4096, 300), (64, 20000)]
SCALES = [1e-3, 1.0, 30.0]
LANES = [1, 2, 4, 8, 16, 32, 64]
MU = 0.5
SEED_BASE = 3000  # (problem (m, n) is seeded with SEED_BASE m + n.  Chosen on the CPU so that every NewtonCG window below is at least MIN_WINDOW or the
                  # whole run -- test_ref_sparse_logistic.py asserts it; the bases tried and what failed are listed there)
WEIGHT_VALUES = LC.WEIGHT_VALUES
MAXG, LONG_ROW, PER_WG = 2048, 2048, 4096  # SPQ_MAXG, SPQ_LONG_ROW and the cut's weight per workgroup (csrc/qn_csr_host.h)
TOL, ITERS, MAX_LS = NC.TOL, NC.ITERS, NC.MAX_LS
MIN_WINDOW, LICENCE, ROUNDING_LICENCE, GPU_TOL, PRODUCT_UNITS = NC.MIN_WINDOW, NC.LICENCE, NC.ROUNDING_LICENCE, NC.GPU_TOL, NC.PRODUCT_UNITS
NEWTON_SHAPES = [(3, 5), (96, 64), (40, 65), (257, 200), (5, 2050), (64, 20000)]
SEARCHES = NC.SEARCHES
CASES = [(m, n, ls) for (m, n) in NEWTON_SHAPES for ls in SEARCHES]
CONVERGENCE = [(96, 64), (40, 65), (257, 200), (64, 20000)]  # BackTracking(1e-4, 0.5) from x0 to ||g||_inf < 1e-7 (asserted on the CPU)
WOLFE = NC.WOLFE
NEG_MU = LC.NEG_MU


def _pattern(rng, m, n, kind):
    """a boolean m x n mask"""
    if (m, n) == (40, 65):
        top, width = (65, 65) if kind == "full" else (64, 64)
        mask = np.zeros((m, n), dtype=bool)
        for i, ln in enumerate(np.round(np.linspace(0, top, m)).astype(int)):
            mask[i, rng.choice(width, size=ln, replace=False)] = True
        return mask
    if (m, n) == (5, 2050):
        mask = rng.random((m, n)) < 0.01
        mask[2, :] = True
        return mask
    if (m, n) == (2050, 7):
        mask = np.zeros((m, n), dtype=bool)
        mask[:, 0] = True
        for i in range(m):
            mask[i, 1 + rng.choice(n - 1, size=2, replace=False)] = True
        return mask
    if (m, n) == (64, 20000):
        mask = np.zeros((m, n), dtype=bool)
        for i in range(m):
            mask[i, rng.choice(n, size=8, replace=False)] = True
        return mask
    density = {(1, 1): 1.0, (3, 5): 0.6, (4096, 300): 0.9}.get((m, n), 0.25)
    return rng.random((m, n)) < density


def to_csr(a, mask, dtype=np.int32):
    """(indptr, indices, data) of the masked entries of a, columns increasing within a row"""
    counts = mask.sum(axis=1)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(dtype)
    rows, cols = np.nonzero(mask)  # (row-major order: the columns of a row increase)
    return indptr, cols.astype(dtype), np.ascontiguousarray(a[rows, cols])


def transpose_csr(indptr, indices, data, n):
    """the CSR of A' by the counting sort csrc/qn_csr_host.h restates: (tptr, tidx, tdata), A's row numbers increasing within a column"""
    m = len(indptr) - 1
    rows = np.repeat(np.arange(m), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=n))]).astype(np.int64)
    return tptr, rows[order], data[order]


def cut(indptr):
    """(G, start, long rows): the device's static cut of one CSR copy -- prefix weight nonzeros + rows, G = ceil(total / 4096) capped at 2048,
    workgroup w starts at the first row whose prefix weight reaches total w // G; rows of more than 2048 entries are long"""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = len(indptr) - 1
    total = int(indptr[-1]) + rows
    g = min(MAXG, max(1, (total + PER_WG - 1) // PER_WG))
    weight = indptr[:rows] + np.arange(rows)
    start = [int(np.searchsorted(weight, total * w // g, side="left")) for w in range(g + 1)]
    start[0], start[g] = 0, rows
    return g, start, [int(i) for i in np.nonzero(np.diff(indptr) > LONG_ROW)[0]]


@functools.lru_cache(maxsize=None)
def problem(m, n, kind="weighted"):
    """dict(indptr, indices, data, a (dense), y, w, mu, x0, v, mask), read-only, computed once.  kind: weighted / unit / edges / full"""
    if kind == "edges":
        base = problem(m, n)
        _, start, _ = cut(base["indptr"])
        w = base["w"].copy()
        owners = [b for b in range(len(start) - 1) if start[b + 1] > start[b]]
        for b in {owners[min(1, len(owners) - 1)], owners[-1]}:
            w[start[b]] = 0.0
            w[start[b + 1] - 1] = 0.0
        w.setflags(write=False)
        return dict(base, w=w)
    rng = np.random.default_rng(SEED_BASE * m + n)
    mask = _pattern(rng, m, n, kind)
    a = np.where(mask, rng.standard_normal((m, n)), 0.0)
    if (m, n) == (2050, 7):
        a[:, 0] = 1.0
    xs = rng.standard_normal(n) / np.sqrt(max(1.0, mask.sum() / m))
    y = np.where(a @ xs + 0.5 * rng.standard_normal(m) >= 0.0, 1.0, -1.0)
    w = np.ones(m) if kind == "unit" else rng.choice(WEIGHT_VALUES, size=m)
    if kind != "unit" and m >= 3 and not np.any(w > 0.0):
        w[m // 2] = 1.0
    x0 = rng.standard_normal(n)
    v = rng.standard_normal(n)
    indptr, indices, data = to_csr(a, mask)
    for arr in (a, y, w, x0, v, indptr, indices, data, mask):
        arr.setflags(write=False)
    return dict(indptr=indptr, indices=indices, data=data, a=a, y=y, w=w, mu=MU, x0=x0, v=v, mask=mask)


_truths = {}


def truth_at(m, n, scale, kind="weighted"):
    """(problem, x, truth_and_bound at x = scale x0 with the problem's v), computed once"""
    key = (m, n, scale, kind)
    if key not in _truths:
        pr = problem(m, n, kind)
        x = scale * pr["x0"]
        _truths[key] = (pr, x, RL.truth_and_bound(pr["a"], pr["y"], pr["w"], pr["mu"], x, pr["v"]))
    return _truths[key]


def saturated_problem():
    """logistic_cases.saturated_problem in CSR: margins -800, +800, +800 (masked) and 0.5"""
    a, y, w, mu, x, z = LC.saturated_problem()
    indptr, indices, data = to_csr(a, a != 0.0)
    return dict(indptr=indptr, indices=indices, data=data, a=a, y=y, w=w, mu=mu, x0=x, v=None), x, z


def csr_eval(pr, x, v=None, d_at=None, t=None):
    """The device's structure in numpy float64: the row pass over A's CSR (margins, coefficients, d, loss), the column pass over the CSR of A' (g and
    ||x||^2; q and v.q for a v), the finish.  dict(f, g, d, q, c).  `d_at`: the point whose d the product uses (default: x).  `t`: a replacement
    (tptr, tidx, tdata) for the transpose.  What the planted faults of tests/test_ref_sparse_logistic.py are planted into."""
    indptr, indices, data = pr["indptr"], pr["indices"], pr["data"]
    m, n = len(indptr) - 1, pr["a"].shape[1]
    tptr, tidx, tdata = t or transpose_csr(indptr, indices, data, n)
    yw = pr["y"] * pr["w"]

    def rows(src):
        return np.array([np.dot(data[indptr[i]:indptr[i + 1]], src[indices[indptr[i]:indptr[i + 1]]]) for i in range(m)])

    def cols(src):
        return np.array([np.dot(tdata[tptr[j]:tptr[j + 1]], src[tidx[tptr[j]:tptr[j + 1]]]) for j in range(n)])

    l, coef, d, _ = RL.row_terms(yw, rows(x))
    out = dict(f=float(np.sum(l)) + 0.5 * pr["mu"] * float(x @ x), g=cols(coef) + pr["mu"] * x, d=d)
    if v is not None:
        dd = d if d_at is None else RL.row_terms(yw, rows(d_at))[2]
        q = cols(dd * rows(v)) + pr["mu"] * v
        out.update(q=q, c=float(v @ q))
    return out


# ---- NewtonCG: the restatement's runs (ref_newton_cg.NewtonCG on ref_logistic of the densified matrix) and their windows ----
def moved_product(pr, mu, seed):
    """logistic_cases.moved_product on this module's problem"""
    a, y, w = pr["a"], pr["y"], pr["w"]
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


def _ordered(pr, mu, order):
    """(fn, product) with every inner product in the given summation order.  numpy: matrix products.  fsum / reversed: each row's dot by cg_cases.DOTS
    over the row's STORED entries -- an absent entry is an exact zero and adds nothing in any order, so this is ref_logistic's function on the
    densified matrix in that order, at the cost of nnz instead of m n"""
    a, y, w = pr["a"], pr["y"], pr["w"]
    if order == "numpy":
        return RL.logistic_fn(a, y, w, mu), RL.logistic_hess_vec_at(a, y, w, mu)
    dot = C.DOTS[order]
    indptr, indices, data = pr["indptr"], pr["indices"], pr["data"]
    m, n = a.shape
    tptr, tidx, tdata = transpose_csr(indptr, indices, data, n)
    yw = y * w

    def rows(src):
        return np.array([dot(data[indptr[i]:indptr[i + 1]], src[indices[indptr[i]:indptr[i + 1]]]) if indptr[i + 1] > indptr[i] else 0.0 for i in range(m)])

    def cols(src):
        return np.array([dot(tdata[tptr[j]:tptr[j + 1]], src[tidx[tptr[j]:tptr[j + 1]]]) if tptr[j + 1] > tptr[j] else 0.0 for j in range(n)])

    def fn(x):
        l, coef, _, _ = RL.row_terms(yw, rows(x))
        return float(dot(l, np.ones(m))) + 0.5 * mu * float(dot(x, x)), cols(coef) + mu * x

    def at_x(x):
        d = RL.row_terms(yw, rows(x))[2]
        return lambda v: cols(d * rows(v)) + mu * v
    return fn, at_x


def line_search(kind, dot=np.dot):
    return NC.line_search(kind, dot)


def run_ref(m, n, ls, iters=ITERS, order="numpy", seed=None, mu=None, tol=TOL, solver=None, max_inner=0):
    """The restatement on one case: (solver object, oracle, status)"""
    pr = problem(m, n)
    mu = pr["mu"] if mu is None else mu
    fn, product = _ordered(pr, mu, order)
    if seed is not None:
        fn, product = C.rounded_otherwise(fn, seed), moved_product(pr, mu, seed)
    o = R.CountingOracle(fn)
    dot = C.DOTS[order]
    s = solver or RN.NewtonCG(tol, pr["x0"], product, max_inner=max_inner, dot=dot)
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


def neg_mu_curvature():
    """(g'Hg, g.g) at x0 of the (3, 5) problem with mu = NEG_MU, in float64: the host's check that rule 4 is met at j = 0"""
    pr = problem(3, 5)
    g = RL.logistic_fn(pr["a"], pr["y"], pr["w"], NEG_MU)(pr["x0"])[1]
    return float(g @ RL.logistic_hess_vec_at(pr["a"], pr["y"], pr["w"], NEG_MU)(pr["x0"])(g)), float(g @ g)


# ---- the rest of the family: the existing restatements on logistic_fn of the densified matrix, licensed the same way ----
FAMILY_WINDOW, FAMILY_TOL, FAMILY_BOX = LC.FAMILY_WINDOW, LC.FAMILY_TOL, LC.FAMILY_BOX
FAMILY_CASES = [("lbfgs", 96, 64), ("lbfgs", 64, 20000), ("cg", 96, 64), ("spg", 96, 64), ("plbfgs", 40, 65)]
family_box = LC.family_box


def family_run(kind, m, n, iters=FAMILY_WINDOW, order="numpy", seed=None):
    """logistic_cases.family_run on this module's problem: LBFGS(5) + StrongWolfe, NonlinearCG("pr+") + StrongWolfe(1e-4, 0.1), SPG + GLLQuadratic in
    a +-0.3 box, ProjectedLBFGS(5) + BackTrackingB in that box: (solver object, status)"""
    import ref_cg as RC
    import ref_lbfgs as RLB
    pr = problem(m, n)
    x0 = pr["x0"]
    fn = _ordered(pr, pr["mu"], order)[0]
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


@functools.lru_cache(maxsize=None)
def family_licence(kind, m, n):
    """(the numpy.dot run, window) of one case of the rest of the family"""
    a = family_run(kind, m, n)[0]
    w = LC._family_agreeing(a, [family_run(kind, m, n, order=order)[0] for order in ("fsum", "reversed")], LICENCE)
    w = min(w, LC._family_agreeing(a, [family_run(kind, m, n, seed=seed)[0] for seed in (1, 2)], ROUNDING_LICENCE))
    return a, min(w, L.above_f_floor(a, "gll" if kind == "spg" else "bt"))
