"""The problems the projected Newton solvers' tests share (tests/test_ref_pnewton.py licenses the windows, tests/test_gpu_pnewton.py uses
them): the seeded synthetic quadratic of tests/spg_cases.py (kappa = 1e2) in the boxes of spg_cases.BOXES, and the log-sum-exp problem of
spg_cases.lse_problem() as a host closure with its analytic Hessian, boxes +-0.3 and infinite.  GLLQuadratic(1e-4, 10), tol 1e-10,
windows of 30 iterations.  (A box of +-0.5 on the quadratics is knife-edge -- f stalls, the line searches run to their cap and the
self-check fails -- and is not used.)"""
import numpy as np

import ref_pnewton as RP
import ref_spg as R
import spg_cases as S

WINDOW = S.WINDOW
TOL = 1e-10
SIZES = (64, 512, 1000)
BOXES = S.BOXES
SOLVERS = ("pn", "spn")
QUAD_CASES = [(s, n, box) for s in SOLVERS for n in SIZES for box in BOXES]
LSE_BOXES = (0.3, float("inf"))
LSE_CASES = [(s, box) for s in SOLVERS for box in LSE_BOXES]
BIG_N = S.BIG_N


def lse_hess_fn(a, c, mu):
    """spg_cases.lse_fn with the analytic Hessian A' (diag(p) - p p') A + mu I."""
    def fn(x):
        z = a @ x + c
        zm = z.max()
        w = np.exp(z - zm)
        sw = w.sum()
        p = w / sw
        ap = a.T @ p
        h = (a.T * p) @ a - np.outer(ap, ap) + mu * np.eye(x.size)
        return zm + np.log(sw) + 0.5 * mu * (x @ x), ap + mu * x, h
    return fn


def run_ref(solver, fn, x0, lb, ub, iters, solve=None, dot=np.dot, max_ls=50, tol=TOL):
    """The restatement on one case: (solver object, oracle, status)."""
    o = RP.HessianOracle(fn)
    if solver == "spn":
        s = RP.SpectralProjectedNewton(tol, x0, o, lb, ub, solve=solve, dot=dot)
    else:
        s = RP.ProjectedNewton(tol, x0, lb, ub, solve=solve, dot=dot)
    ls = R.GLLQuadratic(1e-4, 10, dot=dot)
    status = "ok"
    try:
        s.minimize(ls, o, iters, max_ls)
    except R.MaxIterReached:
        status = "max_iter"
    return s, o, status
