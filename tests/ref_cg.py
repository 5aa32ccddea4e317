"""Pure-Python (numpy float64) restatement of the GPU solver QN_NONLINEAR_CG (kernels csrc/qn_cg.hip.h), on the machine of tests/ref_spg.py: the
same loop (ls_solver.rs:66-133) with tests/ref_wolfe.py's StrongWolfe or ref_spg.BackTracking.  Unbounded: the box is (-inf, +inf).

d+ = beta d - g+ (beta d rounds first, then the difference), with y = g+ - g and d the direction just searched.  The rules, in this order:
    1. the first direction (and the first after `drop_p`) is -g; it is not counted as a restart
    2. restart_every > 0 and that many iterations since the last -g direction: beta = 0
    3. the variant's formula with plain IEEE divisions (a zero denominator gives inf or NaN):
         "fr" g+.g+ / g.g    "pr+" max(0, g+.y / g.g)    "hs+" max(0, g+.y / d.y)    "dy" g+.g+ / d.y
         "hz" max(betaN, eta_k), betaN = (g+.y - ((2 y.y) g+.d) / d.y) / d.y, eta_k = -1 / (sqrt(d.d) min(0.01, sqrt(g.g)))
       (max / min are comparisons, `a if a > b else b`, as in ref_wolfe.py)
    4. beta not finite: beta = 0
    5. Powell's test: |g+.g| >= powell_nu g+.g+ : beta = 0
    6. unless -g+.g+ + beta (g+.d) < 0: beta = 0
Every beta that ends as exactly 0 counts in `restarts`; `updated` is beta != 0.  A zero beta BRANCHES to d = -g.
`dot=` is a parameter as in ref_spg.py.  Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

import ref_spg as R

VARIANTS = ("fr", "pr+", "hs+", "dy", "hz")


def _mx(a, b):
    return a if a > b else b


def _mn(a, b):
    return a if a < b else b


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def beta_formula(variant, gpgp, gpy, dy, gpd, yy, dd, gg):
    """rule 3 alone, on the seven sums it may use"""
    if variant == "fr":
        return _div(gpgp, gg)
    if variant == "pr+":
        return _mx(_div(gpy, gg), 0.0)
    if variant == "hs+":
        return _mx(_div(gpy, dy), 0.0)
    if variant == "dy":
        return _div(gpgp, dy)
    assert variant == "hz"
    corr = _div((2.0 * yy) * gpd, dy)
    beta_n = _div(gpy - corr, dy)
    eta = _div(-1.0, math.sqrt(dd) * _mn(0.01, math.sqrt(gg)))
    return _mx(beta_n, eta)


class NonlinearCG(R._Base):
    def __init__(self, tol, x0, variant="pr+", powell_nu=0.2, restart_every=0, dot=np.dot):
        assert variant in VARIANTS
        self.x = np.array(x0, dtype=np.float64)
        n = self.x.size
        self.lb, self.ub = np.full(n, -R.INF), np.full(n, R.INF)
        self.grad_tol, self.k, self.dot = tol, 0, dot
        self.variant, self.powell_nu, self.restart_every = variant, powell_nu, restart_every
        self.p, self.beta, self.restarts, self.since = None, 0.0, 0, 0
        self.updated, self.betas, self.why = [], [], []  # per iteration: beta != 0, beta, the rule that zeroed it (or None)
        self.directions = []

    def drop_p(self):  # qn_solver_set_cg
        self.p, self.beta, self.since = None, 0.0, 0

    def compute_direction(self, eval_x_k):
        g = eval_x_k[1]
        if self.p is None or self.beta == 0.0:
            d = -g  # a branch: no stale p is multiplied by zero
        else:
            d = self.beta * self.p - g
        self.p = d
        self.directions.append(d)
        return d

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):
        step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
        xk, g, d, dot = self.x, eval_x_k[1], direction, self.dot
        next_iterate = xk + step * direction
        s_k = next_iterate - xk
        gp = oracle(next_iterate)[1]
        y = gp - g
        self.x = next_iterate
        self.last_s_norm = math.sqrt(float(dot(s_k, s_k)))
        gpgp, gpy, dy, gpd = float(dot(gp, gp)), float(dot(gp, y)), float(dot(d, y)), float(dot(gp, d))
        yy, dd, gg, gpg = float(dot(y, y)), float(dot(d, d)), float(dot(g, g)), float(dot(gp, g))
        self.since += 1
        why = None
        if self.restart_every > 0 and self.since >= self.restart_every:
            beta, why = 0.0, "every"
        else:
            beta = beta_formula(self.variant, gpgp, gpy, dy, gpd, yy, dd, gg)
            if beta == 0.0:
                why = "truncated"
            if math.isnan(beta) or math.isinf(beta):
                beta, why = 0.0, "not finite"
            with np.errstate(all="ignore"):
                powell = abs(gpg) >= float(np.float64(self.powell_nu) * np.float64(gpgp))
            if powell:
                beta, why = 0.0, why or "powell"
            if not (-gpgp + beta * gpd < 0.0):
                beta, why = 0.0, why or "descent"
        if beta == 0.0:
            beta = 0.0
            self.restarts += 1
            self.since = 0
        self.beta = beta
        self.updated.append(1 if beta != 0.0 else 0)
        self.betas.append(beta)
        self.why.append(why if beta == 0.0 else None)
        return step
