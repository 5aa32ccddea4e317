"""What tests/test_ref_sparse_multinomial.py (CPU) and tests/test_gpu_sparse_multinomial.py (GPU) share: the sparse softmax-regression problems, the
truths (computed once), the device's structure restated in numpy, and the NewtonCG / family windows by newton_cg_cases' method and constants.

PROBLEMS: sparse_logistic_cases' seeded patterns (m x n, CSR with sorted columns, Gaussian values) with multinomial_cases' label and weight rules:
labels the argmax of a planted W plus Gumbel noise of scale 0.5, weights drawn from {0, 0.5, 1, 3} (some rows are masked), mu = 0.5, x0 and v standard
normal with N = K n entries (class-major); the seed is SEED_BASE m + 31 n + K.  THE TRUTH is ref_multinomial.truth_and_bound on the DENSIFIED matrix:
its bounds hold for a dot in any order and any row length up to n (an absent entry is an exact zero: it adds nothing to any term of a bound), and they
are derived, not measured.  The criterion is |error| / bound <= 1 for f, g, P, q and v'Hv.

SHAPES (m, n, K), each for one way the kernels can go wrong:
    (1, 1, 2)                     the smallest problem
    (3, 5, 3), (40, 65, 5)        K not a power of two; (40, 65, 5): row lengths 0 .. 64 from the first 64 columns (an empty row, an empty column) and
                                  the last class carried by no row
    (96, 64, 16), (17, 8, 17)     a class lane group exactly full, and one past full
    (33, 3, 64), (9, 7, 65)       a full wave of classes, and a second slot
    (7, 9, 300), (5, 4, 600)      K past 256 (one class block of 64 lanes x 4 slots) and past two of them
    (20, 1025, 16)                the shape Multinomial refuses: N_pad is one tile past 16384
    (5, 2050, 4)                  a full row of 2050 entries: a long row of A
    (2050, 7, 3)                  a column of ones over 2050 rows: a long row of A'
    (4096, 300, 4)                density 0.9: more than 256 workgroups in both cuts
    (64, 20000, 5)                8 per row, N = 100 000

THE LICENCE of a window is multinomial_cases' (newton_cg_cases' method and constants, unchanged): three summation orders at LICENCE, two runs with moved
evaluations and products at ROUNDING_LICENCE, f's floor."""
import functools
import zlib

import numpy as np

import cg_cases as C
import lbfgs_cases as L
import multinomial_cases as MC
import newton_cg_cases as NC
import ref_multinomial as RM
import ref_newton_cg as RN
import ref_spg as R
import ref_wolfe as W
import sparse_logistic_cases as SC

SHAPES = [(1, 1, 2), (3, 5, 3), (40, 65, 5), (96, 64, 16), (17, 8, 17), (33, 3, 64), (9, 7, 65), (7, 9, 300), (5, 4, 600), (20, 1025, 16), (5, 2050, 4),
          (2050, 7, 3), (4096, 300, 4), (64, 20000, 5)]
SCALES = [1e-3, 1.0, 30.0]
LANES = SC.LANES
MU = 0.5
SEED_BASE = 4000  # (chosen on the CPU so that every NewtonCG window below is at least MIN_WINDOW or the whole run: test_ref_sparse_multinomial.py asserts it)
WEIGHT_VALUES = MC.WEIGHT_VALUES
TOL, ITERS, MAX_LS = NC.TOL, NC.ITERS, NC.MAX_LS
MIN_WINDOW, LICENCE, ROUNDING_LICENCE, GPU_TOL, PRODUCT_UNITS = NC.MIN_WINDOW, NC.LICENCE, NC.ROUNDING_LICENCE, NC.GPU_TOL, NC.PRODUCT_UNITS
NEWTON_SHAPES = [(96, 16, 4), (40, 13, 5), (257, 40, 5), (64, 20000, 5), (20, 1025, 16)]
SEARCHES = NC.SEARCHES
CASES = [(m, n, k, ls) for (m, n, k) in NEWTON_SHAPES for ls in SEARCHES]
WOLFE = NC.WOLFE
NEG_SHAPE = (3, 5, 3)
NEG_MU = -40.0
KR = 4  # SMN_KR: class slots per lane and class block (csrc/qn_sparse_multinomial.hip.h)


def kp(k):
    """the padded leading dimension of the feature-major copies: the next power of two up to 16, a multiple of 16 above"""
    return max(2, 1 << (k - 1).bit_length()) if k <= 16 else 16 * ((k + 15) // 16)


def auto_lanes(rows, nnz, k):
    """the automatic entry lanes of a copy: the largest power of two at most half the mean row length, capped at 16 lanes per row, class lanes included"""
    lanes = 1
    while lanes < 64 and 2 * lanes <= 0.5 * nnz / rows:
        lanes *= 2
    return max(1, min(lanes, 16 // min(64, 1 << (k - 1).bit_length())))


@functools.lru_cache(maxsize=None)
def problem(m, n, k, kind="weighted"):
    """dict(indptr, indices, data, a (dense), y, w, k, mu, x0, v, mask), read-only, computed once.  kind: weighted / unit / edges"""
    if kind == "edges":
        base = problem(m, n, k)
        _, start, _ = SC.cut(base["indptr"])
        w = base["w"].copy()
        owners = [b for b in range(len(start) - 1) if start[b + 1] > start[b]]
        for b in {owners[min(1, len(owners) - 1)], owners[-1]}:
            w[start[b]] = 0.0
            w[start[b + 1] - 1] = 0.0
        w.setflags(write=False)
        return dict(base, w=w)
    rng = np.random.default_rng(SEED_BASE * m + 31 * n + k)
    mask = SC._pattern(rng, m, n, "weighted")
    a = np.where(mask, rng.standard_normal((m, n)), 0.0)
    if (m, n) == (2050, 7):
        a[:, 0] = 1.0
    wp = rng.standard_normal((k, n)) / np.sqrt(max(1.0, mask.sum() / m))
    y = np.argmax(a @ wp.T + 0.5 * rng.gumbel(size=(m, k)), axis=1).astype(np.int32)
    if (m, n, k) == (40, 65, 5):
        y[y == k - 1] = 0  # the last class is carried by no row
    w = np.ones(m) if kind == "unit" else rng.choice(WEIGHT_VALUES, size=m)
    if kind != "unit" and m >= 3 and not np.any(w > 0.0):
        w[m // 2] = 1.0
    x0 = rng.standard_normal(k * n)
    v = rng.standard_normal(k * n)
    indptr, indices, data = SC.to_csr(a, mask)
    for arr in (a, y, w, x0, v, indptr, indices, data, mask):
        arr.setflags(write=False)
    return dict(indptr=indptr, indices=indices, data=data, a=a, y=y, w=w, k=k, mu=MU, x0=x0, v=v, mask=mask)


_truths = {}


def truth_at(m, n, k, scale, kind="weighted"):
    """(problem, x, truth_and_bound at x = scale x0 with the problem's v), computed once"""
    key = (m, n, k, scale, kind)
    if key not in _truths:
        pr = problem(m, n, k, kind)
        x = scale * pr["x0"]
        _truths[key] = (pr, x, RM.truth_and_bound(pr["a"], pr["y"], pr["w"], k, pr["mu"], x, pr["v"]))
    return _truths[key]


def saturated_problem():
    """multinomial_cases.saturated_problem in CSR: margins spread by 1600"""
    a, y, w, k, mu, x, spread = MC.saturated_problem()
    indptr, indices, data = SC.to_csr(a, a != 0.0)
    return dict(indptr=indptr, indices=indices, data=data, a=a, y=y, w=w, k=k, mu=mu, x0=x, v=None), x, spread


def _spmm(ptr, idx, dat, src, dot):
    """(rows x K): row i of the CSR copy times the skinny matrix src (cols x K), every inner product over the row's STORED entries by `dot`.  A row of
    no entry is 0 and a row of one entry a single product in every order: those are taken together"""
    rows, kk = len(ptr) - 1, src.shape[1]
    out = np.zeros((rows, kk))
    lengths = np.diff(ptr)
    one = np.nonzero(lengths == 1)[0]
    out[one] = dat[ptr[one]][:, None] * src[idx[ptr[one]]]
    for i in np.nonzero(lengths >= 2)[0]:
        d, s = dat[ptr[i]:ptr[i + 1]], src[idx[ptr[i]:ptr[i + 1]]]
        out[i] = [dot(d, np.ascontiguousarray(s[:, c])) for c in range(kk)] if dot is not np.dot else d @ s
    return out


def csr_functions(pr, mu, order="numpy", t=None):
    """(fn, product, probabilities) of the device's structure in float64: x goes to feature-major, the row pass over A's CSR (margins, then
    ref_multinomial.row_terms), the column pass over the CSR of A' (Gt = A'C), back to class-major with + mu x.  Every inner product in the summation
    order `order`.  `t`: a replacement (tptr, tidx, tdata) for the transpose"""
    indptr, indices, data = pr["indptr"], pr["indices"], pr["data"]
    k, n = pr["k"], pr["a"].shape[1]
    m = len(indptr) - 1
    tptr, tidx, tdata = t or SC.transpose_csr(indptr, indices, data, n)
    y, w = pr["y"].astype(np.int64), pr["w"]
    dot = C.DOTS[order]
    ones = np.ones(m)

    def margins(x):
        with np.errstate(over="ignore", invalid="ignore"):
            return _spmm(indptr, indices, data, np.ascontiguousarray(x.reshape(k, n).T), dot)

    def back(ct, x):
        return (_spmm(tptr, tidx, tdata, ct, dot).T + mu * x.reshape(k, n)).ravel()

    def fn(x):
        l, c, _ = RM.row_terms(margins(x), y, w)
        return float(dot(l, ones)) + 0.5 * mu * float(dot(x, x)), back(c, x)

    def probabilities(x):
        return RM.row_terms(margins(x), y, w)[2]

    def at_x(x):
        p = probabilities(x)

        def hv(v):
            u = margins(v)
            with np.errstate(over="ignore", invalid="ignore"):
                ub = np.zeros(m)
                for j in range(k):  # class order
                    ub = ub + p[:, j] * u[:, j]
                tt = (w[:, None] * p) * (u - ub[:, None])
            return back(np.where((w != 0.0)[:, None], tt, 0.0), v)
        return hv
    return fn, at_x, probabilities


def csr_eval(pr, x, v=None, order="numpy", p_at=None, t=None):
    """dict(f, g, p, q, c) of the restatement.  `p_at`: the point whose P the product uses (default: x)"""
    fn, at_x, probabilities = csr_functions(pr, pr["mu"], order, t)
    f, g = fn(x)
    out = dict(f=f, g=g, p=probabilities(x))
    if v is not None:
        q = at_x(x if p_at is None else p_at)(v)
        out.update(q=q, c=float(C.DOTS[order](v, q)))
    return out


# ---- NewtonCG: the restatement's runs (the unmodified ref_newton_cg.NewtonCG on this function) and their windows ----
def line_search(kind, dot=np.dot):
    return NC.line_search(kind, dot)


def moved_product(pr, mu, seed):
    """multinomial_cases.moved_product on this module's problem (the scale by the stored entries)"""
    plain = csr_functions(pr, mu)[1]
    probabilities = csr_functions(pr, mu)[2]
    k, n = pr["k"], pr["a"].shape[1]
    indptr, indices = pr["indptr"], pr["indices"]
    ad = np.abs(pr["data"])
    tptr, tidx, tdata = SC.transpose_csr(indptr, indices, ad, n)
    w = pr["w"]

    def at_x(x):
        hv = plain(x)
        p = probabilities(x)

        def moved(v):
            q = hv(v)
            au = _spmm(indptr, indices, ad, np.ascontiguousarray(np.abs(v).reshape(k, n).T), np.dot)
            scale = _spmm(tptr, tidx, tdata, w[:, None] * p * (au + np.sum(p * au, axis=1)[:, None]), np.dot).T.ravel() + abs(mu) * np.abs(v)
            rng = np.random.default_rng(zlib.crc32(np.ascontiguousarray(v).tobytes()) ^ seed)
            return q + PRODUCT_UNITS * 2.0 ** -53 * rng.uniform(-1.0, 1.0, q.size) * scale
        return moved
    return at_x


def run_ref(m, n, k, ls, iters=ITERS, order="numpy", seed=None, mu=None, tol=TOL, solver=None, max_inner=0):
    """The restatement on one case: (solver object, oracle, status)"""
    pr = problem(m, n, k)
    mu = pr["mu"] if mu is None else mu
    fn, product, _ = csr_functions(pr, mu, order)
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


def neg_mu_curvature():
    """(g'Hg, g.g) at x0 of the NEG_SHAPE problem with mu = NEG_MU, in float64: the host's check that rule 4 is met at j = 0"""
    pr = problem(*NEG_SHAPE)
    fn, at_x, _ = csr_functions(pr, NEG_MU)
    g = fn(pr["x0"])[1]
    return float(g @ at_x(pr["x0"])(g)), float(g @ g)


# ---- the rest of the family: the existing restatements on this function, licensed the same way, at most FAMILY_WINDOW iterations ----
FAMILY_WINDOW, FAMILY_TOL, FAMILY_BOX = MC.FAMILY_WINDOW, MC.FAMILY_TOL, MC.FAMILY_BOX
FAMILY_CASES = [("lbfgs", 96, 16, 4), ("lbfgs", 20, 1025, 16), ("cg", 96, 16, 4), ("spg", 96, 16, 4), ("plbfgs", 40, 13, 5)]
family_box = MC.family_box


def family_run(kind, m, n, k, iters=FAMILY_WINDOW, order="numpy", seed=None):
    """multinomial_cases.family_run on this module's problem: (solver object, status)"""
    import ref_cg as RC
    import ref_lbfgs as RLB
    pr = problem(m, n, k)
    x0 = pr["x0"]
    fn = csr_functions(pr, pr["mu"], order)[0]
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


@functools.lru_cache(maxsize=None)
def family_licence(kind, m, n, k):
    """(the numpy.dot run, window) of one case of the rest of the family"""
    a = family_run(kind, m, n, k)[0]
    w = MC._family_agreeing(a, [family_run(kind, m, n, k, order=order)[0] for order in ("fsum", "reversed")], LICENCE)
    w = min(w, MC._family_agreeing(a, [family_run(kind, m, n, k, seed=seed)[0] for seed in (1, 2)], ROUNDING_LICENCE))
    return a, min(w, L.above_f_floor(a, "gll" if kind == "spg" else "bt"))
