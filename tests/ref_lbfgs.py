"""Pure-Python (numpy float64) restatement of the GPU solver QN_LBFGS / ProjectedLBFGS, on the machine of tests/ref_spg.py: the same loop
(ls_solver.rs:66-133), line searches and projection.  The direction is d = P(x - z) - x with z = H_k g from the last m pairs (s, y).

z comes from the TWO-LOOP RECURSION (Nocedal 1980) by default -- deliberately not the compact form the GPU kernels use, so the GPU is checked
against an independent formulation; `direction="compact"` is the compact form of Byrd, Nocedal and Schnabel (1994) for the self-checks of
tests/test_ref_lbfgs.py.  Shared with the GPU solver: the commit rule (a pair is kept only when s.y > DBL_EPSILON y.y), the safeguard (g.z <= 0
or not finite with stored pairs: the memory is cleared, z = g, `resets` counts it) and the unit-scaling switch (gamma = 1).
Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

import ref_spg as R

EPS = float(np.finfo(np.float64).eps)


def two_loop(pairs, g, gamma, dot):
    q = np.array(g, dtype=np.float64)
    alphas = []
    for s, y in reversed(pairs):  # newest first
        a = float(dot(s, q)) / float(dot(y, s))
        q = q - a * y
        alphas.append(a)
    r = gamma * q
    for (s, y), a in zip(pairs, reversed(alphas)):  # oldest first
        b = float(dot(y, r)) / float(dot(y, s))
        r = r + (a - b) * s
    return r


def compact(pairs, g, gamma, dot):
    """z = gamma g + S u + gamma Y v with R = triu(S'Y), D = diag(s_i.y_i), p = S'g, q = Y'g, v = -R^-1 p, u = R^-T [(D + gamma Y'Y) R^-1 p - gamma q]"""
    k = len(pairs)
    sy = np.array([[float(dot(si, yj)) for _, yj in pairs] for si, _ in pairs])
    yy = np.array([[float(dot(yi, yj)) for _, yj in pairs] for _, yi in pairs])
    p = np.array([float(dot(s, g)) for s, _ in pairs])
    q = np.array([float(dot(y, g)) for _, y in pairs])
    r = np.triu(sy)
    w = np.zeros(k)
    for i in range(k - 1, -1, -1):
        w[i] = (p[i] - float(r[i, i + 1:] @ w[i + 1:])) / r[i, i]
    rhs = (np.diag(sy) * w + gamma * (yy @ w)) - gamma * q
    u = np.zeros(k)
    for i in range(k):
        u[i] = (rhs[i] - float(r[:i, i] @ u[:i])) / r[i, i]
    z = gamma * np.array(g, dtype=np.float64)
    for (s, y), ui, wi in zip(pairs, u, w):
        z = z + ui * s
        z = z + (gamma * -wi) * y
    return z


class LBFGS(R._Base):
    def __init__(self, tol, x0, lower_bound, upper_bound, m=5, unit_scaling=False, dot=np.dot, direction="two_loop"):
        self.lb, self.ub = np.asarray(lower_bound, dtype=np.float64), np.asarray(upper_bound, dtype=np.float64)
        self.x = R.box_projection(np.asarray(x0, dtype=np.float64), self.lb, self.ub)
        self.grad_tol, self.k, self.m, self.unit, self.dot = tol, 0, m, unit_scaling, dot
        self.hg = {"two_loop": two_loop, "compact": compact}[direction]
        self.pairs, self.resets, self.gamma, self.updated = [], 0, 1.0, []

    def stored_pairs(self):
        return len(self.pairs)

    def compute_direction(self, eval_x_k):
        g = eval_x_k[1]
        z = g
        if self.pairs:
            s, y = self.pairs[-1]
            with np.errstate(all="ignore"):
                self.gamma = 1.0 if self.unit else float(self.dot(s, y)) / float(self.dot(y, y))
                z = self.hg(self.pairs, g, self.gamma, self.dot)
                gz = float(self.dot(g, z))
            if not (gz > 0.0) or math.isinf(gz):
                self.pairs, self.resets, self.gamma, z = [], self.resets + 1, 1.0, g
        else:
            self.gamma = 1.0
        direction = R.box_projection(self.x - z, self.lb, self.ub)
        return direction - self.x

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):
        step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
        xk = self.x
        next_iterate = xk + step * direction
        s_k = next_iterate - xk
        y_k = oracle(next_iterate)[1] - eval_x_k[1]
        self.x = next_iterate
        self.last_s_norm = math.sqrt(float(self.dot(s_k, s_k)))
        commit = float(self.dot(s_k, y_k)) > EPS * float(self.dot(y_k, y_k))
        if commit:
            self.pairs.append((s_k, y_k))
            if len(self.pairs) > self.m:
                self.pairs.pop(0)
        self.updated.append(1 if commit else 0)
        return step
