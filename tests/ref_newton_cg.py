"""Pure-Python (numpy float64) restatement of the GPU solver QN_NEWTON_CG (kernels csrc/qn_newton_cg.hip.h, qn_lse_hv.hip.h), on the machine of
tests/ref_spg.py: the same loop (ls_solver.rs:66-133) with ref_spg.BackTracking or tests/ref_wolfe.py's StrongWolfe.  Unbounded: the box is
(-inf, +inf).  The accepted point is not evaluated by the update step: the next loop top's call is that evaluation.

ONE DIRECTION, the rules in the device's order, operation for operation:
    1. p = softmax(A x + c), gbar = A'p                               (`hess_vec_at(x)` returns the product v -> H v made with them)
    2. z = 0, r = g, p = g, gg = g.g, rr = gg, j = 0, eta = min(eta_max, sqrt(sqrt(gg)))    (min is a comparison)
    3. q = H p = A'(p o (A p)) - gbar (p . (A p)) + mu p, kappa = p.q
    4. unless kappa > 0 and finite: neg_curv += 1; z = g if j == 0; the loop ends
    5. alpha = rr / kappa; z += alpha p, r -= alpha q (the products round first); j += 1; rr' = r.r; (g.z is summed in the same pass)
    6. sqrt(rr') <= eta sqrt(gg): the loop ends ("tol"); else j == max_inner: it ends ("cap")
    7. beta = rr' / rr; p = r + beta p (the product rounds first); rr = rr'; back to 3
    8. g.z > 0 and finite, or else z = g and fallbacks += 1 (not tested after rule 4 at j = 0: z is g); d = -z
`dot=` is a parameter as in ref_spg.py.  Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

import ref_spg as R


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def lse_hess_vec_at(a, c, mu):
    """x -> (v -> H(x) v) of f = log sum exp(A x + c) + mu/2 ||x||^2, in the device's association: (A'w - ubar gbar) + mu v"""
    at = np.ascontiguousarray(a.T)

    def at_x(x):
        z = a @ x + c
        e = np.exp(z - z.max())
        p = e / e.sum()
        gbar = at @ p

        def hv(v):
            w = p * (a @ v)
            return (at @ w - float(np.sum(w)) * gbar) + mu * v
        return hv
    return at_x


class NewtonCG(R._Base):
    def __init__(self, tol, x0, hess_vec_at, eta_max=0.5, max_inner=0, dot=np.dot):
        self.x = np.array(x0, dtype=np.float64)
        n = self.x.size
        self.lb, self.ub = np.full(n, -R.INF), np.full(n, R.INF)
        self.grad_tol, self.k, self.dot = tol, 0, dot
        self.hess_vec_at, self.eta_max, self.cap = hess_vec_at, eta_max, (max_inner if max_inner > 0 else min(n, 100))
        self.inner, self.why, self.directions = [], [], []  # per direction: j_k, the exit reason, d
        self.hv_passes = self.neg_curv = self.fallbacks = 0

    def compute_direction(self, eval_x_k):
        g, dot = eval_x_k[1], self.dot
        hv = self.hess_vec_at(self.x)
        z, r, p = np.zeros_like(g), g.copy(), g.copy()
        gg = float(dot(g, g))
        rr, j = gg, 0
        sqgg = math.sqrt(gg)
        s4 = math.sqrt(sqgg)
        eta = s4 if s4 < self.eta_max else self.eta_max
        zg, gz = False, 0.0
        while True:
            q = hv(p)
            self.hv_passes += 1
            kappa = float(dot(p, q))
            if not (kappa > 0.0) or math.isinf(kappa):
                self.neg_curv += 1
                zg = j == 0
                why = "negcurv"
                break
            alpha = _div(rr, kappa)
            z = z + alpha * p
            r = r - alpha * q
            j += 1
            rrn, gz = float(dot(r, r)), float(dot(g, z))
            rr_old, rr = rr, rrn
            if math.sqrt(rrn) <= eta * sqgg:
                why = "tol"
                break
            if j >= self.cap:
                why = "cap"
                break
            beta = _div(rrn, rr_old)
            p = r + beta * p
        if zg:
            d = -g
        elif not (gz > 0.0) or math.isinf(gz):
            self.fallbacks += 1
            why += "+fallback"
            d = -g
        else:
            d = -z
        self.inner.append(j)
        self.why.append(why)
        self.directions.append(d)
        return d

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):
        step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
        self.x = self.x + step * direction
        return step
