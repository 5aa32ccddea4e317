"""The problems the ExactQuadratic tests share (tests/test_ref_exact.py licenses the windows, tests/test_gpu_exact.py uses them): sparse_cases' matrices
-- tri, arrow, band(n, 20) as SparseQuadratic, and tri once more as a dense Quadratic -- at n = 7 and 2050, b and x0 as there, tol 1e-10, at most
30 iterations, under every method the search is admitted for and refresh_every = 1, 0, 3.  Every restatement run is made once and kept.

    method   "pgd" ProjectedGradientDescent, "spg" SpectralProjectedGradient, "lbfgs" LBFGS(m = 5), "cg-fr" / "cg-pr+" / "cg-hz" NonlinearCG: free;
             "pgd-box", "spg-box", "plbfgs": the same three in a box of half-width BOX[(matrix, n)] around 0, where the step is capped at 1

THE LICENCE of a window: the case runs with numpy.dot, with math.fsum of the products, and with every dot product AND every row of Q summed in
reversed order.  The window ends at the first iteration where the iterates differ by more than 1e-11 max(1, ||x||), t by more than 1e-11 |t|, or a
decision differs: the cap t = 1, a CG restart (beta == 0), an L-BFGS commit, a forced refresh, or the way the run ends.  A window is at least
MIN_WINDOW iterations, or the whole run where every order converges in the same, smaller number of iterations (`whole_run`).  The GPU sums in a fourth order and is
compared inside the window at 1e-9 max(1, ||x||)."""
import functools

import numpy as np

import lbfgs_cases as LC
import ref_cg as RC
import ref_exact as RE
import ref_lbfgs as RL
import ref_spg as R
import sparse_cases as SC
import spg_cases as S

WINDOW = 30
MIN_WINDOW = 8
TOL = 1e-10
LICENCE = 1e-11
SIZES = (7, 2050)
REFRESH = (1, 0, 3)
OBJECTIVES = ("tri", "arrow", "band", "dense")
FREE_METHODS = ("pgd", "spg", "lbfgs", "cg-fr", "cg-pr+", "cg-hz")
BOX_METHODS = ("pgd-box", "spg-box", "plbfgs")
LBFGS_M = 5
# the half-width of the box per problem.  sparse_cases' +-0.05 takes every coordinate of the start (0.5 .. 1.5) onto the upper face; at n = 7 the solution
# lies there too and the run converges at once, and at n = 2050 ProjectedLBFGS's second direction does not descend (the run ends there: an error-path
# case of the GPU tests).  The half-widths below are sparse_cases.WIDE_BOX's -- under the start's range, so the start is projected, and wide enough that
# coordinates leave the face.
BOX = {(a, n): SC.WIDE_BOX[("tri" if a in ("band", "dense") else a, n)] for a in OBJECTIVES for n in SIZES}
BOX[("band", 15)] = 1.0
# REPLACED: ProjectedLBFGS at n = 7.  With an active face its direction d = P(x - H g) - x stops descending (include/qn_hip.h says so for the bounded
# variant) and every n = 7 run ends with "not a descent direction" after 5 or 6 iterations, in every box tried (half-widths 0.5 .. 2): no window of 8,
# and no convergence.  In its place: band at n = 15 (odd, one workgroup, padding) with half-width 1, which converges in 26 iterations with windows of
# 15 and 16; the n = 2050 runs end the same way after 12 iterations (tri, arrow, dense: the window is those 12) or run to the cap (band).  The n = 7
# run on tri is kept as the GPU tests' case of "ProjectedLBFGS met with g.d >= 0": NOT_DESCENT_CASE, whose three orders agree on all 5 iterations.
CASES = ([(m, a, n, r) for m in FREE_METHODS for a in OBJECTIVES for n in SIZES for r in REFRESH] +
         [(m, a, n, r) for m in ("pgd-box", "spg-box") for a in OBJECTIVES for n in SIZES for r in REFRESH] +
         [("plbfgs", a, 2050, r) for a in OBJECTIVES for r in REFRESH] + [("plbfgs", "band", 15, r) for r in REFRESH])
NOT_DESCENT_CASE = ("plbfgs", "tri", 7, 1)


def rev_dot(a, b):
    return float(np.dot(a[::-1], b[::-1]))


ORDERS = {"numpy": (np.dot, False), "fsum": (R.fsum_dot, False), "reversed": (rev_dot, True)}


@functools.lru_cache(maxsize=None)
def matrix(name, n):
    if name == "band":
        return SC.band(n, 20)
    return SC.tri(n) if name == "dense" else SC.matrix(name, n)


def box_of(method, name, n):
    return S.bounds(n, BOX[(name, n)]) if method in BOX_METHODS else LC.free_box(n)


def make_solver(method, x0, lb, ub, oracle, dot):
    if method in ("pgd", "pgd-box"):
        return R.ProjectedGradientDescent(TOL, x0, lb, ub)
    if method in ("spg", "spg-box"):
        return R.SpectralProjectedGradient(TOL, x0, oracle, lb, ub, dot=dot)
    if method in ("lbfgs", "plbfgs"):
        return RL.LBFGS(TOL, x0, lb, ub, m=LBFGS_M, dot=dot)
    return RC.NonlinearCG(TOL, x0, variant=method[3:], dot=dot)


def run_ref(case, iters=WINDOW, order="numpy", tol=None, csr=None, b=None, x0=None):
    """The restatement on one case: (solver, line search, oracle, status); status "ok" | "max_iter" | "not_descent" | "curvature" """
    method, name, n, r = case
    dot, reverse = ORDERS[order]
    csr = matrix(name, n) if csr is None else csr
    b = SC.rhs(n) if b is None else b
    x0 = SC.start(n) if x0 is None else x0
    lb, ub = box_of(method, name, n)
    o = RE.ExactOracle(SC.quadratic_fn(csr, b, reverse), lambda v: SC.matvec(csr, v, reverse), r)
    ls = RE.ExactQuadratic(o, bounded=method in BOX_METHODS, dot=dot)
    s = make_solver(method, x0, lb, ub, o, dot)
    if tol is not None:
        s.grad_tol = tol
    try:
        status = RE.minimize(s, ls, o, iters)
    except R.MaxIterReached:
        status = "max_iter"
    except RE.NotDescent:
        status = "not_descent"
    except RE.NonPositiveCurvature:
        status = "curvature"
    return s, ls, o, status


@functools.lru_cache(maxsize=None)
def ref_case(case):
    return run_ref(case)


def decisions(s, ls, k):
    """what iteration k decided, beside the numbers: the cap, the refresh, and the method's own branch"""
    h = ls.history[k]
    own = None
    if isinstance(s, RC.NonlinearCG):
        own = s.updated[k]
    elif isinstance(s, RL.LBFGS):
        own = s.updated[k]
    return h["capped"], h["refresh"], own


@functools.lru_cache(maxsize=None)
def licence(case):
    """(window, whole_run, worst spread of x inside it): the leading iterations on which the three summation orders agree"""
    a, la, oa, sa = ref_case(case)
    others = [run_ref(case, order=o) for o in ("fsum", "reversed")]
    n_it = len(a.trace)
    window, worst = n_it, 0.0
    for s, ls, o, st in others:
        w = 0
        for k in range(min(n_it, len(s.trace))):
            xa, xb = a.trace_x[k], s.trace_x[k]
            spread = float(np.linalg.norm(xa - xb)) / max(1.0, float(np.linalg.norm(xa)))
            ta, tb = a.trace[k]["t"], s.trace[k]["t"]
            if spread > LICENCE or abs(ta - tb) > LICENCE * abs(ta) or decisions(a, la, k) != decisions(s, ls, k):
                break
            worst = max(worst, spread)
            w = k + 1
        window = min(window, w)
    same_end = all(st == sa and len(s.trace) == n_it and o.forced == oa.forced for s, _, o, st in others)
    whole_run = window == n_it and same_end and sa == "ok"
    return window, whole_run, worst


def window(case):
    return licence(case)[0]


# ---- the 2-D five-point Laplacian plus a shift: the problem of "the point of the feature", of examples/exact_cg_example.cpp and of tools/bench_exact.py ----
@functools.lru_cache(maxsize=None)
def laplacian(m, shift=0.05):
    n = m * m
    idx = np.arange(n, dtype=np.int64).reshape(m, m)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0 + shift)]
    for p, q in ((idx[1:, :], idx[:-1, :]), (idx[:-1, :], idx[1:, :]), (idx[:, 1:], idx[:, :-1]), (idx[:, :-1], idx[:, 1:])):
        rows.append(p.ravel())
        cols.append(q.ravel())
        vals.append(np.full(p.size, -1.0))
    return SC.from_triplets(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def laplacian_rhs(n):
    """b = 1, as examples/exact_cg_example.cpp"""
    return np.ones(n)


@functools.lru_cache(maxsize=None)
def laplacian_cg(order="numpy", m=64, tol=1e-8, cap=2000):
    """NonlinearCG("fr") + ExactQuadratic(0) from x0 = 0 on the m x m Laplacian plus 0.05 I: (iterations, status, forced refreshes)"""
    n = m * m
    s, _, o, status = run_ref(("cg-fr", "lap", n, 0), iters=cap, order=order, tol=tol, csr=laplacian(m), b=laplacian_rhs(n), x0=np.zeros(n))
    return len(s.trace), status, o.forced


# ---- convergence confirmation: a tolerance the recurrence gradient passes and the true gradient does not ----
# CG on tri(2050) with refresh_every = 0 and tol = 0: in every summation order the recurrence gradient keeps falling by a factor of about 8 per 10
# iterations (9e-15 at iteration 170, 1e-15 at 180, 2e-17 at 200) while the true gradient Q x - b stalls at its rounding floor, 4.9e-14 .. 5.3e-14 from
# iteration 170 on (eps ||Q|| ||x|| is 5e-14 here).  CONFIRM_TOL = 5e-15 lies between the two: a factor of 10 under the floor.
CONFIRM_CASE = ("cg-fr", "tri", 2050, 0)
CONFIRM_TOL = 5e-15
CONFIRM_CAP = 200
CONFIRM_FIRST_PASS = 174  # the iteration whose loop top first sees a recurrence gradient under the tolerance, in all three orders; with the rule the runs
#                           go on to 179 .. 184 iterations with 4 .. 8 forced refreshes and end on a TRUE gradient under the tolerance (restarting the
#                           recurrence from true gradients lowers the floor)


@functools.lru_cache(maxsize=None)
def confirm_ref(order="numpy"):
    return run_ref(CONFIRM_CASE, iters=CONFIRM_CAP, order=order, tol=CONFIRM_TOL)
