"""Pure-Python (numpy float64) restatement of the reference's two bounded second-order solvers, on top of tests/ref_spg.py (whose
`_Base.minimize`, `GLLQuadratic` and `CountingOracle` it reuses), the CPU checker of QN_PROJECTED_NEWTON / QN_SPECTRAL_PROJECTED_NEWTON:

    src/newton/projected_newton.rs:14-47     ProjectedNewton::new, next_iterate_too_close, gradient_next_iterate_too_close
    src/newton/projected_newton.rs:64-80     compute_direction: P(x - H^-1 g) - x
    src/newton/projected_newton.rs:95-110    has_converged: s_norm, then y_norm, then the projected gradient
    src/newton/projected_newton.rs:112-140   update_next_iterate
    src/newton/spn.rs:22-58                  SpectralProjectedNewton::new (lambda0), with_lambdas
    src/newton/spn.rs:76-91                  compute_direction: P(x - lambda H^-1 g) - x
    src/newton/spn.rs:93-150                 has_converged, update_next_iterate (the Barzilai-Borwein update)

The oracle returns (f, g) with the Hessian beside it (`Eval`).  The solve z = H^-1 g is a parameter (`solve=`): by default `hessian.cholesky().unwrap().solve(g)` on the LOWER
TRIANGLE of H, as nalgebra does -- for n <= 8 in nalgebra's own operation order (column Cholesky by axpys, column-oriented forward and
row-oriented backward substitution), above that by LAPACK; `lu_solve` is the other route of the summation-order self-check.  `dot=` is a
parameter as in ref_spg.py.  Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

import ref_spg as R

try:
    import scipy.linalg as _sl
except ImportError:  # (numpy alone: slower triangular solves, the same checks)
    _sl = None


class NotPositiveDefinite(Exception):
    """Cholesky::new returned None: the reference panics on the unwrap."""


class Eval(tuple):
    """FuncEvalMultivariate::from((f, g)).with_hessian(h): the (f, g) pair ref_spg.py's line searches unpack, with the Hessian beside it."""

    def __new__(cls, f, g, h):
        self = super().__new__(cls, (f, g))
        self.h = h
        return self


class HessianOracle(R.CountingOracle):
    """Wraps fn(x) -> (f, g, H); counts the calls of the reference's sequence."""

    def __call__(self, x):
        self.calls += 1
        f, g, h = self.fn(np.array(x, dtype=np.float64))
        return Eval(float(f), np.asarray(g, dtype=np.float64), h)


def _nalgebra_cholesky(h):
    n = h.shape[0]
    m = np.tril(np.array(h, dtype=np.float64))
    for j in range(n):
        for k in range(j):
            factor = -m[j, k]
            m[j:, j] = factor * m[j:, k] + m[j:, j]
        diag = m[j, j]
        if not diag > 0.0:
            raise NotPositiveDefinite()
        denom = math.sqrt(diag)
        m[j, j] = denom
        m[j + 1:, j] = m[j + 1:, j] / denom
    return m


def _nalgebra_solve(l, g, dot):
    n = l.shape[0]
    b = np.array(g, dtype=np.float64)
    for i in range(n):  # solve_lower_triangular: column-oriented
        coeff = b[i] / l[i, i]
        b[i] = coeff
        b[i + 1:] = (-coeff) * l[i + 1:, i] + b[i + 1:]
    for i in range(n - 1, -1, -1):  # ad_solve_lower_triangular: a dot product per row
        d = float(dot(l[i + 1:, i], b[i + 1:])) if i + 1 < n else 0.0
        b[i] = (b[i] - d) / l[i, i]
    return b


class CholeskySolve:
    """`hessian.cholesky().unwrap().solve(g)`: the lower triangle only.  The factor of the SAME matrix object is kept (a quadratic's Hessian)."""

    def __init__(self, dot=np.dot):
        self.dot, self._h, self._l, self.factorisations = dot, None, None, 0

    def __call__(self, h, g):
        if h is not self._h:
            self.factorisations += 1
            if h.shape[0] <= 8:
                self._l = _nalgebra_cholesky(h)
            else:
                hl = np.tril(h)
                try:
                    self._l = np.linalg.cholesky(hl + np.tril(h, -1).T)
                except np.linalg.LinAlgError:
                    raise NotPositiveDefinite() from None
            self._h = h
        l = self._l
        if h.shape[0] <= 8:
            return _nalgebra_solve(l, g, self.dot)
        if _sl is not None:
            return _sl.solve_triangular(l, _sl.solve_triangular(l, g, lower=True), lower=True, trans="T")
        return np.linalg.solve(l.T, np.linalg.solve(l, g))


class LUSolve:
    """The other route of the self-check: a pivoted LU of the symmetric matrix the lower triangle stands for."""

    def __init__(self):
        self._h, self._f = None, None

    def __call__(self, h, g):
        if h is not self._h:
            full = np.tril(h) + np.tril(h, -1).T
            self._f = _sl.lu_factor(full) if _sl is not None else np.linalg.inv(full)
            self._h = h
        return _sl.lu_solve(self._f, g) if _sl is not None else self._f @ g


class ProjectedNewton(R._Base):
    def __init__(self, grad_tol, x0, lower_bound, upper_bound, solve=None, dot=np.dot):  # projected_newton.rs:27-46
        self.lb, self.ub = np.asarray(lower_bound, dtype=np.float64), np.asarray(upper_bound, dtype=np.float64)
        self.x = R.box_projection(np.asarray(x0, dtype=np.float64), self.lb, self.ub)
        self.grad_tol, self.k, self.dot = grad_tol, 0, dot
        self.solve = solve or CholeskySolve(dot)
        self.s_norm = self.y_norm = None
        self.ended_by = None

    def next_iterate_too_close(self):  # :15-20
        return self.s_norm is not None and self.s_norm < self.grad_tol

    def gradient_next_iterate_too_close(self):  # :21-26
        return self.y_norm is not None and self.y_norm < self.grad_tol

    def has_converged(self, eval_x_k):  # :95-110
        if self.next_iterate_too_close():
            self.ended_by = "s_norm"
            return True
        if self.gradient_next_iterate_too_close():
            self.ended_by = "y_norm"
            return True
        if float(np.max(np.abs(self.projected_gradient(eval_x_k)))) < self.grad_tol:
            self.ended_by = "projected_gradient"
            return True
        return False

    def compute_direction(self, eval_x_k):  # :64-80
        direction = self.x - self.solve(eval_x_k.h, eval_x_k[1])
        direction = R.box_projection(direction, self.lb, self.ub)
        return direction - self.x

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):  # :112-140
        step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
        next_iterate = self.x + step * direction
        s = next_iterate - self.x
        self.s_norm = math.sqrt(float(self.dot(s, s)))
        y = oracle(next_iterate)[1] - eval_x_k[1]
        self.y_norm = math.sqrt(float(self.dot(y, y)))
        self.last_s_norm, self.last_y_norm = self.s_norm, self.y_norm
        self.x = next_iterate
        self.y_norms = getattr(self, "y_norms", []) + [self.y_norm]
        return step


class SpectralProjectedNewton(R.SpectralProjectedGradient):
    def __init__(self, grad_tol, x0, oracle, lower_bound, upper_bound, solve=None, dot=np.dot):  # spn.rs:28-58 (== spg.rs:28-58)
        super().__init__(grad_tol, x0, oracle, lower_bound, upper_bound, dot=dot)
        self.solve = solve or CholeskySolve(dot)

    def compute_direction(self, eval_x_k):  # spn.rs:76-91
        direction = self.x - self.lam * self.solve(eval_x_k.h, eval_x_k[1])
        direction = R.box_projection(direction, self.lb, self.ub)
        return direction - self.x
    # update_next_iterate: spn.rs:111-149 is spg.rs:106-144 statement for statement (R.SpectralProjectedGradient's)


def quadratic_fn(q, b):
    """f = 1/2 x'Qx - b'x, g = Qx - b, H = Q (the same object every call: the solve keeps its factor)."""
    base = R.quadratic_fn(q, b)

    def fn(x):
        f, g = base(x)
        return f, g, q
    return fn
