"""Pure-Python (numpy float64) restatement of the reference's Broyden / BroydenB, the CPU checker of the GPU solver QN_BROYDEN.  Sequential
semantics, statement by statement:

    src/ls_solver.rs:66-111                      minimize, evaluate_x_k
    src/quasi_newton/broyden.rs:42-121           Broyden: compute_direction, has_converged, update_next_iterate
    src/quasi_newton/broyden_b.rs                BroydenB: x0 projected in new, d = P(x - H g) - x, the same update
    src/line_search/morethuente.rs               MoreThuente        (tests/ref_python.py's restatement, by import)
    src/line_search/morethuente_b.rs             MoreThuenteB       (the same search behind the clip of t_max, :185-201)
    src/line_search/backtracking.rs, _b.rs       BackTracking, BackTrackingB (tests/ref_spg.py's restatements, by import)

The update, broyden.rs:115-118, as written:

    hy = H y ; numerator = ((s - hy) s') H ; H += numerator / s.dot(y)

i.e. H + c a w' with a = s - H y, w = H' s (a ROW vector times H), c = 1 / s.y.  Not the textbook formula; H+ y = s does not hold.

Two switches sample the floating-point orders an implementation may take:
    update="literal"    the n x n outer product (a s') first, then the n x n by n x n product with H, then the division (the reference)
    update="factored"   w = H' s first, then a_i * w_j, scaled by c = 1 / s.y (what a one-pass kernel does)
    matvec="dot"        numpy.dot / @ for every mat-vec and dot product
    matvec="fsum"       math.fsum of the products (correctly rounded sums) for every mat-vec and dot product of the solver; the n^3 product of
                        update="literal" stays numpy's
Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

import ref_python as rp
import ref_spg as rs

INF = float("inf")


class MaxIterReached(Exception):
    pass


class OutOfDomain(Exception):
    pass


def _dot(matvec):
    return np.dot if matvec == "dot" else rs.fsum_dot


def _gemv(h, x, matvec):
    if matvec == "dot":
        return h @ x
    return np.array([math.fsum((row * x).tolist()) for row in h])


class MoreThuente:
    def __init__(self):
        self.mt = rp.MoreThuente()
        self.trials = 0

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):
        f_k, g_k = eval_x_k

        def orc(p):
            f, g = oracle(np.array(p, dtype=np.float64))
            return f, [float(v) for v in g]
        return self.mt.compute_step_len([float(v) for v in x_k], f_k, [float(v) for v in g_k], [float(v) for v in direction_k], orc, max_iter)


class MoreThuenteB(MoreThuente):
    def __init__(self, lower_bound, upper_bound):
        super().__init__()
        self.lb, self.ub = np.asarray(lower_bound, dtype=np.float64), np.asarray(upper_bound, dtype=np.float64)

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):  # morethuente_b.rs:185-201
        cand = INF
        for i in range(len(x_k)):
            di = float(direction_k[i])
            v = INF
            if di > 0.0:
                v = (self.ub[i] - x_k[i]) / di
            elif di < 0.0:
                v = (self.lb[i] - x_k[i]) / di
            cand = rs.rmin(float(v), cand)
        self.mt.t_max = rs.rmin(self.mt.t_max, cand)
        return super().compute_step_len(x_k, eval_x_k, direction_k, oracle, max_iter)


BackTracking = rs.BackTracking
BackTrackingB = rs.BackTrackingB


def broyden_update(h, s, y, update="literal", matvec="dot"):
    """broyden.rs:115-118 on a copy of h"""
    dot = _dot(matvec)
    hy = _gemv(h, y, matvec)
    a = s - hy
    den = float(dot(s, y))
    if update == "literal":
        numerator = np.outer(a, s) @ h  # (n^3: the matrix product stays numpy's in both settings of `matvec`)
        return h + numerator / den
    w = _gemv(h.T, s, matvec)  # w = H' s
    c = 1.0 / den
    return h + c * np.outer(a, w)


class Broyden:
    def __init__(self, tol, x0, update="literal", matvec="dot"):  # broyden.rs:27-40
        self.x = np.array(x0, dtype=np.float64)
        n = self.x.size
        self.h = np.eye(n)
        self.k, self.tol, self.s_norm, self.y_norm = 0, tol, None, None
        self.update, self.matvec = update, matvec
        self.lb = self.ub = None

    def next_iterate_too_close(self):
        return self.s_norm is not None and self.s_norm < self.tol

    def gradient_next_iterate_too_close(self):
        return self.y_norm is not None and self.y_norm < self.tol

    def compute_direction(self, eval_x_k):  # :42-49
        return -_gemv(self.h, eval_x_k[1], self.matvec)

    def has_converged(self, eval_x_k):  # :64-76
        if self.next_iterate_too_close():
            return True
        if self.gradient_next_iterate_too_close():
            return True
        g = eval_x_k[1]
        return math.sqrt(float(_dot(self.matvec)(g, g))) < self.tol

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):  # :78-121
        dot = _dot(self.matvec)
        step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
        next_iterate = self.x + step * direction
        s = next_iterate - self.x
        self.s_norm = math.sqrt(float(dot(s, s)))
        y = oracle(next_iterate)[1] - eval_x_k[1]
        self.y_norm = math.sqrt(float(dot(y, y)))
        self.x = next_iterate
        self.updated = False
        if self.next_iterate_too_close():
            return step
        if self.gradient_next_iterate_too_close():
            return step
        self.h = broyden_update(self.h, s, y, self.update, self.matvec)
        self.updated = True
        return step

    def minimize(self, line_search, oracle, max_iter_solver, max_iter_line_search, callback=None):  # ls_solver.rs:66-111
        self.k = 0
        self.trace, self.trace_x = [], []
        while max_iter_solver > self.k:
            c0 = oracle.calls
            oracle.at_loop_top = True
            eval_x_k = oracle(self.x)
            if math.isnan(eval_x_k[0]) or math.isinf(eval_x_k[0]):
                raise OutOfDomain()
            if self.has_converged(eval_x_k):
                return
            direction = self.compute_direction(eval_x_k)
            gnorm = math.sqrt(float(_dot(self.matvec)(eval_x_k[1], eval_x_k[1])))
            t = self.update_next_iterate(line_search, eval_x_k, oracle, direction, max_iter_line_search)
            self.trace.append(dict(f=eval_x_k[0], gnorm=gnorm, t=t, n_evals=oracle.calls - c0, s_norm=self.s_norm, y_norm=self.y_norm,
                                   updated=int(self.updated)))
            self.trace_x.append(self.x.copy())
            self.k += 1
            if callback is not None:
                callback(self)
        raise MaxIterReached()


class BroydenB(Broyden):
    def __init__(self, tol, x0, lower_bound, upper_bound, update="literal", matvec="dot"):  # broyden_b.rs:44-66
        super().__init__(tol, x0, update, matvec)
        self.lb, self.ub = np.asarray(lower_bound, dtype=np.float64), np.asarray(upper_bound, dtype=np.float64)
        self.x = rs.box_projection(self.x, self.lb, self.ub)

    def compute_direction(self, eval_x_k):  # :68-79
        direction = self.x - _gemv(self.h, eval_x_k[1], self.matvec)
        direction = rs.box_projection(direction, self.lb, self.ub)
        return direction - self.x


class MemoOracle(rs.CountingOracle):
    """Counts the calls of the reference's sequence (`calls`) and, beside them, the evaluations an evaluate-each-distinct-point-once solver
    (qn_oracle.memoize = 1) performs (`evals`): that solver keeps the evaluation at the current iterate and the last trial evaluated, so a call is
    answered without an evaluation when its point is bit for bit one of the two.  A line search that projects its trials (BackTrackingB) takes
    nothing from the memo: there only the loop-top call, at the point `oracle(next_iterate)` has just evaluated, is answered from it."""

    def __init__(self, fn, projected_ls=False):
        super().__init__(fn)
        self.evals, self.projected_ls, self.at_loop_top = 0, projected_ls, False
        self._cur = self._last = None

    def __call__(self, x):
        key = np.array(x, dtype=np.float64).tobytes()
        top, self.at_loop_top = self.at_loop_top, False
        if self.projected_ls:
            hit = top and key == self._last
        else:
            hit = key == self._cur or key == self._last
        if not hit:
            self.evals += 1
        self._last = key
        if top:
            self._cur = key
        return super().__call__(x)
