"""The problems the StrongWolfe tests share (tests/test_ref_wolfe.py licenses the windows, tests/test_gpu_wolfe.py uses them), taken from
lbfgs_cases.py, spg_cases.py and pnewton_cases.py: the kappa = 1e2 synthetic quadratic, the log-sum-exp problem, the double-well chain of the
example device closure.  tol 1e-10, at most 30 iterations, line searches of at most 50 trials.  Every restatement run is made once and kept.

A case is (solver, oracle, n, m, box[, line-search settings]):
    solver  "lbfgs" | "spg" | "pgd" | "pn"
    oracle  "host" / "quad" (the synthetic quadratic as a closure / on the device), "lse" (log-sum-exp), "chain" (the device closure's function),
            "concave" / "reject" (lbfgs_cases.concave_mixed_fn / reject_fn, host closures at n = 2 / 3)
    m       L-BFGS memory (0 for the others)
    box     None, or the half-width of the solver's box; then the line search holds the same box ("boxed form")

The WINDOW of a case is not a table: window(case) runs the restatement with numpy.dot, with math.fsum of the products and with the reversed
summation order and returns the number of leading iterations in which the three took the same decisions, agreed to 1e-11 in x and t, and stayed
above lbfgs_cases.above_f_floor.  tests/test_ref_wolfe.py asserts that every one is at least 8 iterations long."""
import functools

import numpy as np

import lbfgs_cases as LC
import pnewton_cases as PC
import ref_lbfgs as RL
import ref_pnewton as RP
import ref_spg as R
import ref_wolfe as RW
import spg_cases as S

TOL = 1e-10
ITERS = 30
MAX_LS = 50
LICENCE = 1e-11
MIN_WINDOW = 8

C2 = (("c2", 0.1),)  # a tight curvature condition: more trials per search, and dcstep's cases 2 and 3 with them
TMAX8 = (("t_max", 8.0),)  # the concave slice is unbounded below: its searches end on stp = stpmax
CASES = [
    ("lbfgs", "host", 7, 1, None),
    ("lbfgs", "quad", 2050, 5, None),
    ("lbfgs", "lse", 2050, 17, None),
    ("lbfgs", "chain", 1000, 5, None, C2),
    ("lbfgs", "concave", 2, 5, None, TMAX8),
    ("spg", "chain", 1000, 0, 1.5, C2),
    ("pgd", "lse", 64, 0, None, C2),
    ("pgd", "concave", 2, 0, None, TMAX8),
    ("pn", "lse", 64, 0, None),
]
BOX_CASES = [("lbfgs", "chain", 1000, 5, 1.5, C2), ("lbfgs", "chain", 1000, 1, 1.5)]  # ProjectedLBFGS, the search holding the solver's box
# NOT USED, and why: projected gradient and SPG on the kappa = 1e2 quadratic.  A cubic through two points of a quadratic lands on the exact line
# minimiser, so phi' at the second trial is +-1e-16 and the stage switch (`phi' >= 0`) is decided by the summation order: the three restatement runs
# disagree on bit 30 of ls_cases in the first iterations (same steps, same iterates).  The quadratic stays in through L-BFGS, whose searches
# after the first accept t = 1.


def rev_dot(a, b):
    return float(np.dot(a[::-1], b[::-1]))


@functools.lru_cache(maxsize=None)
def problem(oracle, n):
    """(fn, x0) -- fn returns (f, g)"""
    if oracle == "chain":
        a, c, x0, _, _ = S.chain_problem(n)
        return S.chain_fn(a, c), x0
    if oracle == "reject":
        return LC.reject_fn, np.array(LC.REJECT_X0)
    if oracle == "concave":
        return LC.concave_mixed_fn, np.array(LC.CONCAVE_X0)
    if oracle == "lse" and n == 64:
        a, c, mu, x0, _, _ = S.lse_problem()
        return S.lse_fn(a, c, mu), x0
    return LC.oracle_fn(oracle, n)


def box_of(n, box):
    return LC.free_box(n) if box is None else S.bounds(n, box)


def line_search(lb, ub, boxed, dot=np.dot, **kw):
    return RW.StrongWolfe(lower_bound=lb if boxed else None, upper_bound=ub if boxed else None, dot=dot, **kw)


def run_ref(case, dot=np.dot, iters=ITERS, max_ls=MAX_LS, direction="two_loop", ls_kw=None):
    """The restatement on one case: (solver object, line search, oracle, status)."""
    solver, oracle, n, m, box = case[:5]
    fn, x0 = problem(oracle, n)
    lb, ub = box_of(n, box)
    ls = line_search(lb, ub, box is not None, dot, **dict(case[5] if len(case) > 5 else (), **(ls_kw or {})))
    if solver == "pn":
        a, c, mu, _, _, _ = S.lse_problem()
        o = RP.HessianOracle(PC.lse_hess_fn(a, c, mu))
        s = RP.ProjectedNewton(TOL, x0, lb, ub, dot=dot)
    else:
        o = R.CountingOracle(fn)
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


def agreement(a, la, others):
    """leading iterations in which every other run took a's decisions and agrees with it to LICENCE in x and t; and the worst spread inside them"""
    n, worst = len(a.trace), 0.0
    for o, lo in others:
        n = min(n, len(o.trace))
    for k in range(n):
        w = 0.0
        for o, lo in others:
            same = (a.trace[k]["n_evals"] == o.trace[k]["n_evals"] and a.trace[k]["ls_iters"] == o.trace[k]["ls_iters"]
                    and la.history[k]["ls_cases"] == lo.history[k]["ls_cases"]
                    and getattr(a, "updated", [0] * n)[k] == getattr(o, "updated", [0] * n)[k])
            if not same:
                return k, worst
            w = max(w, float(np.linalg.norm(a.trace_x[k] - o.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k]))),
                    abs(a.trace[k]["t"] - o.trace[k]["t"]) / abs(a.trace[k]["t"]))
        if w > LICENCE:
            return k, worst
        worst = max(worst, w)
    return n, worst


@functools.lru_cache(maxsize=None)
def licence(case):
    """(window, worst spread inside it)"""
    a, la, _, _ = ref_case(case)
    others = [run_ref(case, dot=R.fsum_dot)[:2], run_ref(case, dot=rev_dot)[:2]]
    if case[0] == "lbfgs":
        others.append(run_ref(case, direction="compact")[:2])
    n, worst = agreement(a, la, others)
    return max(0, min(n, LC.above_f_floor(a, "wolfe"))), worst


def window(case):
    return licence(case)[0]
