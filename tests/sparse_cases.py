"""The problems the sparse-quadratic tests share (tests/test_ref_sparse.py licenses the windows, tests/test_gpu_sparse.py uses them): min 1/2 x'Qx - b'x
with a sparse SPD Q in CSR.  numpy only.  The CSR product is restated as np.bincount(rows, weights=vals * x[cols], minlength=n) -- one sum per row
in storage order; `reverse=True` adds every row's products in the opposite order (the summation-order check of the licences).

    tri(n)      tridiag(-1, 2.04, -1): eigenvalues in (0.04, 4.04), kappa = 101 at n = 2050
    arrow(n)    tri(n) plus a dense first row and column, Q_0j = Q_j0 = 0.5 / n (1 + j % 7) / 7 for j >= 2, Q_00 = 3.04 (kappa = 101 at n = 2050)
    band(n, h)  half-width h, entries -1 / (1 + |i - j|), diagonal = row sum of magnitudes + 0.04 (strictly diagonally dominant)
    b = default_rng(5).standard_normal(n),  x0_i = 0.5 + (0.3819660112501051 i) mod 1

Sizes follow the kernel (csrc/qn_sparse.hip.h): n = 7 (one workgroup, odd, rows shorter than every lanes-per-row), 2050 (several workgroups, the
last one ragged; arrow's first row is longer than the long-row threshold of 2048), 2^21 + 2 (the regular workgroups' row loop wraps many times).
tol 1e-10, at most 30 iterations, line searches of at most 50 trials, as lbfgs_cases.  Every restatement run is made once and kept."""
import functools

import numpy as np

import lbfgs_cases as LC
import ref_lbfgs as RL
import ref_spg as R
import ref_wolfe as RW
import spg_cases as S
import wolfe_cases as W

WINDOW = 30
TOL = 1e-10
MAX_LS = 50
LICENCE = 1e-11
MATRICES = ("tri", "arrow")
SIZES = (7, 2050)
BIG_N, BIG_M, BIG_WINDOW = (1 << 21) + 2, 3, 5


# ---- matrices: (indptr, indices, data), int64 indices, columns increasing inside a row ----
def from_triplets(n, rows, cols, vals):
    rows, cols, vals = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return indptr, cols, vals


@functools.lru_cache(maxsize=None)
def tri(n):
    i = np.arange(n, dtype=np.int64)
    rows = np.concatenate([i, i[1:], i[:-1]])
    cols = np.concatenate([i, i[:-1], i[1:]])
    vals = np.concatenate([np.full(n, 2.04), np.full(n - 1, -1.0), np.full(n - 1, -1.0)])
    return from_triplets(n, rows, cols, vals)


@functools.lru_cache(maxsize=None)
def arrow(n):
    indptr, cols, vals = tri(n)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    vals = vals.copy()
    vals[(rows == 0) & (cols == 0)] = 3.04
    j = np.arange(2, n, dtype=np.int64)
    w = 0.5 / n * (1 + j % 7) / 7
    z = np.zeros(j.size, dtype=np.int64)
    return from_triplets(n, np.concatenate([rows, z, j]), np.concatenate([cols, j, z]), np.concatenate([vals, w, w]))


@functools.lru_cache(maxsize=None)
def band(n, h):
    i = np.arange(n, dtype=np.int64)
    rows, cols, vals = [], [], []
    diag = np.full(n, 0.04)
    for d in range(1, min(h, n - 1) + 1):
        v = 1.0 / (1 + d)
        rows += [i[d:], i[:-d]]
        cols += [i[:-d], i[d:]]
        vals += [np.full(n - d, -v), np.full(n - d, -v)]
        diag[d:] += v
        diag[:-d] += v
    return from_triplets(n, np.concatenate(rows + [i]), np.concatenate(cols + [i]), np.concatenate(vals + [diag]))


def matrix(name, n):
    return {"tri": tri, "arrow": arrow}[name](n)


def rhs(n):
    return np.random.default_rng(5).standard_normal(n)


def start(n):
    return 0.5 + (0.3819660112501051 * np.arange(n, dtype=np.float64)) % 1.0


def row_index(indptr):
    return np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))


def matvec(csr, x, reverse=False):
    """Q x: one sum per row, the products added in storage order (reverse: in the opposite order)"""
    indptr, cols, vals = csr
    rows, w = row_index(indptr), vals * x[cols]
    if reverse:
        rows, w = rows[::-1], w[::-1]
    return np.bincount(rows, weights=w, minlength=indptr.size - 1)


def dense(csr):
    indptr, cols, vals = csr
    n = indptr.size - 1
    q = np.zeros((n, n))
    q[row_index(indptr), cols] = vals
    return q


def quadratic_fn(csr, b, reverse=False):
    """f = 1/2 x'Qx - b'x, g = Qx - b on the host, written as ref_spg.quadratic_fn is"""
    rows = row_index(csr[0])
    cols, vals = csr[1], csr[2]
    n = b.size
    if reverse:
        rows, cols, vals = rows[::-1], cols[::-1], vals[::-1]

    def fn(x):
        qx = np.bincount(rows, weights=vals * x[cols], minlength=n)
        return 0.5 * float(x @ qx) - float(b @ x), qx - b
    return fn


@functools.lru_cache(maxsize=None)
def problem(name, n, reverse=False):
    """(fn, x0) of one matrix at size n"""
    return quadratic_fn(matrix(name, n), rhs(n), reverse), start(n)


def rev_dot(a, b):
    return float(np.dot(a[::-1], b[::-1]))


# ---- cases ----
# (solver, ls, m, matrix, n, box[, line-search settings]): solver "lbfgs" | "spg" | "pgd"; ls "gll" | "bt" | "btb" | "wolfe"; m: the L-BFGS memory (0
# otherwise); box: None or the half-width of the solver's box (BackTrackingB holds the same box); settings: as wolfe_cases, (("t_max", 0.5),)
LBFGS_CASES = [("lbfgs", ls, m, a, n, None) for ls in ("gll", "bt") for m in (1, 5, 32) for a in MATRICES for n in SIZES]
# StrongWolfe with its default settings.  At n = 2050 the licensed window is EMPTY: the first trial t = 1 overshoots, the second is the cubic through
# two points of a quadratic -- the exact line minimiser --, so phi' there is +-1e-13 and the stage switch (`phi' >= 0`, bit 30 of ls_cases) is decided
# by the summation order: the restatement's own runs disagree on it in iteration 0 (same steps, same iterates; wolfe_cases.py meets the same on its
# quadratic).  TMAX_HALF caps the step at 0.5, beyond the first search's minimiser (0.38): every search is then one trial with a decided sign, and
# those cases license 14 to 30 iterations.  At n = 7 the first search accepts t = 1 and the default settings license 9 iterations.
TMAX_HALF = (("t_max", 0.5),)
WOLFE_CASES = ([("lbfgs", "wolfe", 5, a, n, None) for a in MATRICES for n in SIZES] +
               [("lbfgs", "wolfe", 5, a, 2050, None, TMAX_HALF) for a in MATRICES])
WOLFE_KNIFE_EDGE = [("lbfgs", "wolfe", 5, a, 2050, None) for a in MATRICES]
FIRST_ORDER_CASES = [(s, ls, 0, a, n, None) for s, ls in (("spg", "gll"), ("pgd", "bt")) for a in MATRICES for n in SIZES]
FREE_CASES = LBFGS_CASES + WOLFE_CASES + FIRST_ORDER_CASES
# ProjectedLBFGS.  GLLQuadratic in spg_cases' box of +-0.05 at n = 2050 (at n = 7 that box takes every coordinate of the start AND of the solution
# onto its upper face: the run converges at once with active = n).  BackTracking / BackTrackingB stall in it after one iteration (the projected
# quasi-Newton direction stops descending and the searches run to their cap); WIDE_BOX holds the half-width chosen for those two per problem, below
# the start's range [0.5, 1.5) -- so the start is projected onto the upper face -- and wide enough that the restatement's window is 5 iterations with
# 0 < active bounds < n at its end (0.5 and 0.4 give windows of 2 to 4, 1.5 and wider leave nothing active at n = 7).
BOX = 0.05
WIDE_BOX = {("tri", 7): 0.75, ("arrow", 7): 1.0, ("tri", 2050): 1.0, ("arrow", 2050): 1.0}
BOX_CASES = ([("lbfgs", "gll", 5, a, 2050, BOX) for a in MATRICES] +
             [("lbfgs", ls, 5, a, n, WIDE_BOX[(a, n)]) for ls in ("bt", "btb") for a in MATRICES for n in SIZES])
ALL_CASES = FREE_CASES + BOX_CASES
# windows shorter than min(leading commits, f floor, 30).  (bt, m = 1, arrow, 2050): tests/test_ref_sparse.py's self-check finds the formulations
# 1.07e-11 apart at iteration 29.  GLLQuadratic in the +-0.05 box: at iteration 7 the restatement's own runs report different norms of the
# projected gradient (0.39 against 1.35: x + 1.0 (P(x - z) - x) lands ON a bound in one summation order and one ulp beside it in another, and the
# projected gradient drops a coordinate only when x == bound exactly) while their iterates agree to 1e-15 -- the norm is compared on the GPU, so the
# window ends in front of it.  (From iteration 25 on the direction no longer descends, the interpolation returns a negative step and the iterate
# leaves the box: the method's own behaviour, which qn_hip.h states for the bounded variant.)
SHORTER = {("lbfgs", "bt", 1, "arrow", 2050, None): 28, ("lbfgs", "gll", 5, "tri", 2050, BOX): 7, ("lbfgs", "gll", 5, "arrow", 2050, BOX): 7}


def box_slack(box):
    """how far rounding may take an iterate outside the box: x_next = x + t d with d = P(x - z) - x is the subtraction and the sum (t = 1 is exact,
    t < 1 stays inside), each rounded by at most u = 2^-53 times a magnitude of at most 2 box and box: 3 u box, stated as 4 u box"""
    return 4.0 * 2.0 ** -53 * box


def box_of(n, box):
    return LC.free_box(n) if box is None else S.bounds(n, box)


def run_ref(case, iters=WINDOW, dot=np.dot, direction="two_loop", reverse=False, max_ls=MAX_LS):
    """The restatement on one case: (solver object, line search, oracle, status)"""
    solver, ls_kind, m, name, n, box = case[:6]
    fn, x0 = problem(name, n, reverse)
    lb, ub = box_of(n, box)
    o = R.CountingOracle(fn)
    if ls_kind == "wolfe":
        ls = RW.StrongWolfe(lower_bound=None, upper_bound=None, dot=dot, **dict(case[6] if len(case) > 6 else ()))
    else:
        ls = LC.line_search(ls_kind, lb, ub, dot)
    if solver == "lbfgs":
        s = RL.LBFGS(TOL, x0, lb, ub, m=m, dot=dot, direction=direction)
    elif solver == "spg":
        s = R.SpectralProjectedGradient(TOL, x0, o, lb, ub, dot=dot)
    else:
        s = R.ProjectedGradientDescent(TOL, x0, lb, ub)
    status = "ok"
    try:
        s.minimize(ls, o, iters, max_ls)
    except R.MaxIterReached:
        status = "max_iter"
    except RW.NotDescent:
        status = "not_descent"
    return s, ls, o, status


@functools.lru_cache(maxsize=None)
def ref_case(case):
    return run_ref(case)


def other_runs(case):
    """the formulations a window is licensed against: reversed dot products, every row of Q summed in reversed order, and for L-BFGS the compact form
    (StrongWolfe: math.fsum dot products too, as wolfe_cases.licence)"""
    runs = [run_ref(case, dot=rev_dot), run_ref(case, reverse=True)]
    if case[0] == "lbfgs":
        runs.append(run_ref(case, direction="compact"))
    if case[1] == "wolfe":
        runs.append(run_ref(case, dot=R.fsum_dot))
    return runs


@functools.lru_cache(maxsize=None)
def wolfe_licence(case):
    """(window, worst spread inside it) by wolfe_cases.agreement: the leading iterations with the same decisions (ls_cases among them) and 1e-11 agreement"""
    a, la, _, _ = ref_case(case)
    n, worst = W.agreement(a, la, [r[:2] for r in other_runs(case)])
    return max(0, min(n, LC.above_f_floor(a, "wolfe"))), worst


def window(case):
    a, _, _, _ = ref_case(case)
    if case[1] == "wolfe":
        return wolfe_licence(case)[0]
    w = min(LC.above_f_floor(a, case[1]), SHORTER.get(case, WINDOW), len(a.trace))
    if case[0] == "lbfgs":
        w = min(w, LC.leading_commits(a))
    return max(1, w)


@functools.lru_cache(maxsize=None)
def ref_big():
    """tri(2^21 + 2), LBFGS(m = 3) + BackTracking, 5 iterations"""
    return run_ref(("lbfgs", "bt", BIG_M, "tri", BIG_N, None), iters=BIG_WINDOW)
