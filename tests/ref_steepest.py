"""Pure-Python (numpy float64) restatement of the reference's PnormDescent, CoordinateDescent and NoSearch, the CPU checker of the GPU solvers
QN_PNORM_DESCENT / QN_COORDINATE_DESCENT and of QN_LS_NO_SEARCH.  Sequential semantics, statement by statement:

    src/ls_solver.rs:66-111                              minimize, evaluate_x_k
    src/steepest_descent/pnorm_descent.rs:30-85          PnormDescent: compute_direction, has_converged, update_next_iterate
    src/steepest_descent/coordinate_descent.rs:24-94     CoordinateDescent: the same, with the (position, max_value) fold AS WRITTEN
    src/steepest_descent/gradient_descent.rs:24-82       GradientDescent (NoSearch's third partner in the tests)
    src/line_search/nosearch.rs                          NoSearch: the step is 1.0, the oracle is not called
    src/line_search/morethuente.rs                       MoreThuente  (tests/ref_python.py's restatement, by import)
    src/line_search/backtracking.rs                      BackTracking (tests/ref_spg.py's restatement, by import)

One switch samples the floating-point orders an implementation may take, as tests/ref_broyden.py's does:
    matvec="dot"    n <= 5: the reference's literal order -- the column sweep y = P[:,0] g_0; y += P[:,j] g_j with two roundings per term, and
                    nalgebra's dot product; larger n: numpy.dot / @
    matvec="fsum"   math.fsum of the products (correctly rounded sums) for the mat-vec and every dot product
Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

import ref_python as rp
import ref_spg as rs
from ref_broyden import MemoOracle  # noqa: F401  (the call / evaluation counts of memoize = 0 / 1)

INF = float("inf")
SMALL_N = 5


class MaxIterReached(Exception):
    pass


class OutOfDomain(Exception):
    pass


def literal_dot(a, b):
    return rp.dot([float(v) for v in a], [float(v) for v in b])


def _dot(matvec, n):
    if matvec == "fsum":
        return rs.fsum_dot
    return literal_dot if n <= SMALL_N else np.dot


def _gemv(m, x, matvec):
    n = len(x)
    if matvec == "fsum":
        return np.array([math.fsum((row * x).tolist()) for row in m])
    if n <= SMALL_N:
        return np.array(rp.gemv([[float(v) for v in row] for row in m], [float(v) for v in x]))
    return m @ x


class NoSearch:  # nosearch.rs:3-15
    trials = 0

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):
        return 1.0


class MoreThuente:
    """ref_python's More-Thuente; its dot products are nalgebra's (exact order at n <= 5) or, with matvec="fsum", correctly rounded"""

    def __init__(self, matvec="dot"):
        self.mt = rp.MoreThuente()
        self.matvec = matvec

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):
        f_k, g_k = eval_x_k

        def orc(p):
            f, g = oracle(np.array(p, dtype=np.float64))
            return f, [float(v) for v in g]
        if self.matvec == "fsum":
            saved = rp.dot
            rp.dot = lambda a, b: math.fsum([u * v for u, v in zip(a, b)])
            try:
                return self.mt.compute_step_len([float(v) for v in x_k], f_k, [float(v) for v in g_k], [float(v) for v in direction_k], orc, max_iter)
            finally:
                rp.dot = saved
        return self.mt.compute_step_len([float(v) for v in x_k], f_k, [float(v) for v in g_k], [float(v) for v in direction_k], orc, max_iter)


def BackTracking(c1, beta, n, matvec="dot"):
    return rs.BackTracking(c1, beta, dot=_dot(matvec, n))


def inf_norm(g):  # grad.iter().fold(NEG_INFINITY, |acc, x| x.abs().max(acc)): Rust's f64::max returns the non-NaN operand
    acc = -INF
    for v in g:
        acc = rs.rmax(abs(float(v)), acc)
    return acc


def coordinate_fold(g):
    """coordinate_descent.rs:31-41: (position, max_value), replaced on a STRICT `g.abs() > max` -- the first index of the largest magnitude wins,
    a NaN never does, and nothing above 0.0 leaves (0, 0.0)"""
    idx, mx = 0, 0.0
    for i, v in enumerate(g):
        a = abs(float(v))
        if a > mx:
            idx, mx = i, a
    return idx, mx


def signum(v):  # f64::signum: 1.0 for +0.0 and everything positive, -1.0 for -0.0 and everything negative, NaN for NaN
    if v != v:
        return v
    return math.copysign(1.0, v)


class _SteepestBase:
    def __init__(self, grad_tol, x0, matvec="dot"):
        self.grad_tol, self.x, self.k, self.matvec = grad_tol, np.array(x0, dtype=np.float64), 0, matvec

    def has_converged(self, eval_x_k):
        return inf_norm(eval_x_k[1]) < self.grad_tol

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):
        step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
        self.x = self.x + step * direction
        return step

    def minimize(self, line_search, oracle, max_iter_solver, max_iter_line_search, callback=None):  # ls_solver.rs:66-111
        self.k = 0
        self.trace, self.trace_x, self.trace_d = [], [], []
        while max_iter_solver > self.k:
            c0 = oracle.calls
            oracle.at_loop_top = True
            eval_x_k = oracle(self.x)
            if math.isnan(eval_x_k[0]) or math.isinf(eval_x_k[0]):
                raise OutOfDomain()
            if self.has_converged(eval_x_k):
                return
            direction = self.compute_direction(eval_x_k)
            t = self.update_next_iterate(line_search, eval_x_k, oracle, direction, max_iter_line_search)
            self.trace.append(dict(f=eval_x_k[0], gnorm=inf_norm(eval_x_k[1]), t=t, n_evals=oracle.calls - c0))
            self.trace_x.append(self.x.copy())
            self.trace_d.append(np.array(direction))
            self.k += 1
            if callback is not None:
                callback(self)
        raise MaxIterReached()


class GradientDescent(_SteepestBase):
    def compute_direction(self, eval_x_k):  # gradient_descent.rs:24-30
        return -eval_x_k[1]


class PnormDescent(_SteepestBase):
    def __init__(self, grad_tol, x0, inverse_p, matvec="dot"):  # pnorm_descent.rs:20-27
        super().__init__(grad_tol, x0, matvec)
        self.inverse_p = np.array(inverse_p, dtype=np.float64)

    def compute_direction(self, eval_x_k):  # :35  Ok(-&self.inverse_p * eval.g())
        return _gemv(-self.inverse_p, eval_x_k[1], self.matvec)


class CoordinateDescent(_SteepestBase):
    def compute_direction(self, eval_x_k):  # :30-44
        grad_k = eval_x_k[1]
        position, max_value = coordinate_fold(grad_k)
        direction_k = np.zeros(len(grad_k))
        direction_k[position] = -signum(max_value)
        return direction_k
