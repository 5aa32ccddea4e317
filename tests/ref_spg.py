"""Pure-Python (numpy float64) restatement of the reference's first-order family, the CPU checker of the GPU solvers QN_SPG /
QN_PROJECTED_GRADIENT.  Sequential semantics, statement by statement:

    src/ls_solver.rs:66-133                                 minimize, evaluate_x_k, projected_gradient
    src/steepest_descent/spg.rs:28-145                      SpectralProjectedGradient
    src/steepest_descent/projected_gradient_descent.rs      ProjectedGradientDescent
    src/line_search/gll_quadratic.rs                        GLLQuadratic
    src/line_search/backtracking.rs, backtracking_b.rs      BackTracking, BackTrackingB
    src/line_search/mod.rs:25-37                            sufficient_decrease

Element-wise numpy arithmetic on float64 rounds once per operation and never fuses a*b+c, like rustc.  The dot product is a parameter
(`dot=`): numpy.dot by default, math.fsum of the products for the summation-order self-check.  Test infrastructure: the product does not
import this file.
"""
import math

import numpy as np

INF = float("inf")


class MaxIterReached(Exception):
    pass


class OutOfDomain(Exception):
    pass


def fsum_dot(a, b):
    return math.fsum((a * b).tolist())


def rmax(a, b):  # Rust f64::max: the non-NaN operand
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def rmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def box_projection(x, lb, ub):
    return np.minimum(np.maximum(x, lb), ub)


class CountingOracle:
    """Wraps fn(x) -> (f, g); counts the calls of the reference's sequence."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, x):
        self.calls += 1
        f, g = self.fn(np.array(x, dtype=np.float64))
        return float(f), np.asarray(g, dtype=np.float64)


class GLLQuadratic:
    def __init__(self, c1, m, dot=np.dot):  # gll_quadratic.rs:13-23
        self.c1, self.m, self.f_previous, self.sigma1, self.sigma2, self.dot = c1, m, [], 0.1, 0.9, dot
        self.branches = []  # per inner iteration: "accept", "halve", "interp", "half_interp"

    def with_sigmas(self, sigma1, sigma2):  # :24-28
        self.sigma1, self.sigma2 = sigma1, sigma2
        return self

    def append_new_f(self, f):  # :30-35
        if len(self.f_previous) == self.m:
            self.f_previous.pop(0)
        self.f_previous.append(f)

    def f_max(self):  # :37-43
        acc = -INF
        for x in self.f_previous:
            acc = rmax(x, acc)
        return acc

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):  # :53-99
        f_k, g_k = eval_x_k
        self.append_new_f(f_k)
        t = 1.0
        f_max = self.f_max()
        i = 0
        self.trials = 0
        gd = float(self.dot(g_k, direction_k))
        while max_iter > i:
            x_kp1 = x_k + t * direction_k
            f_kp1, _ = oracle(x_kp1)
            self.trials += 1
            if f_kp1 - f_max <= self.c1 * t * gd:  # :73, mod.rs:35
                self.branches.append("accept")
                return t
            if t <= 0.1:  # :78-80
                self.branches.append("halve")
                t *= 0.5
            else:
                t_tmp = -0.5 * t * t * gd / (f_kp1 - f_k - t * gd)  # :83-84
                if t_tmp > self.sigma1 and t_tmp < self.sigma2 * t:  # :85-87
                    self.branches.append("interp")
                    t = t_tmp
                else:
                    self.branches.append("half_interp")
                    t = t_tmp * 0.5  # :91
            i += 1
        return t


class BackTracking:
    def __init__(self, c1, beta, dot=np.dot):
        self.c1, self.beta, self.dot = c1, beta, dot

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):  # backtracking.rs:20-58
        f_k, g_k = eval_x_k
        t, i = 1.0, 0
        self.trials = 0
        gd = float(self.dot(g_k, direction_k))
        while max_iter > i:
            f_kp1, _ = oracle(x_k + t * direction_k)
            self.trials += 1
            if math.isnan(f_kp1) or math.isinf(f_kp1):
                t *= self.beta
                continue
            if f_kp1 - f_k <= self.c1 * t * gd:
                return t
            t *= self.beta
            i += 1
        return t


class BackTrackingB:
    def __init__(self, c1, beta, lower_bound, upper_bound, dot=np.dot):
        self.c1, self.beta, self.dot = c1, beta, dot
        self.lb, self.ub = np.asarray(lower_bound, dtype=np.float64), np.asarray(upper_bound, dtype=np.float64)

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):  # backtracking_b.rs:52-90
        f_k, _ = eval_x_k
        t, i = 1.0, 0
        self.trials = 0
        while max_iter > i:
            x_kp1 = box_projection(x_k + t * direction_k, self.lb, self.ub)
            f_kp1, _ = oracle(x_kp1)
            self.trials += 1
            if math.isnan(f_kp1) or math.isinf(f_kp1):
                t *= self.beta
                continue
            diff = x_kp1 - x_k
            if f_kp1 - f_k <= (-self.c1 / t) * float(self.dot(diff, diff)):  # :32-33
                return t
            t *= self.beta
            i += 1
        return t


class _Base:
    def projected_gradient(self, eval_x_k):  # ls_solver.rs:121-133
        g = np.array(eval_x_k[1], dtype=np.float64)
        g[((self.x == self.lb) & (g > 0.0)) | ((self.x == self.ub) & (g < 0.0))] = 0.0
        return g

    def has_converged(self, eval_x_k):
        pg = self.projected_gradient(eval_x_k)
        return float(np.max(np.abs(pg))) < self.grad_tol

    def minimize(self, line_search, oracle, max_iter_solver, max_iter_line_search, callback=None):  # ls_solver.rs:66-111
        self.k = 0
        self.trace, self.trace_x = [], []
        while max_iter_solver > self.k:
            c0 = oracle.calls
            eval_x_k = oracle(self.x)
            if math.isnan(eval_x_k[0]) or math.isinf(eval_x_k[0]):
                raise OutOfDomain()
            if self.has_converged(eval_x_k):
                return
            direction = self.compute_direction(eval_x_k)
            gnorm = float(np.max(np.abs(self.projected_gradient(eval_x_k))))
            t = self.update_next_iterate(line_search, eval_x_k, oracle, direction, max_iter_line_search)
            self.trace.append(dict(f=eval_x_k[0], gnorm=gnorm, t=t, n_evals=oracle.calls - c0, ls_iters=line_search.trials,
                                   s_norm=getattr(self, "last_s_norm", 0.0)))
            self.trace_x.append(self.x.copy())
            self.k += 1
            if callback is not None:
                callback(self)
        raise MaxIterReached()


class ProjectedGradientDescent(_Base):
    def __init__(self, grad_tol, x0, lower_bound, upper_bound):  # projected_gradient_descent.rs:15-32
        self.lb, self.ub = np.asarray(lower_bound, dtype=np.float64), np.asarray(upper_bound, dtype=np.float64)
        self.x = box_projection(np.asarray(x0, dtype=np.float64), self.lb, self.ub)
        self.grad_tol, self.k = grad_tol, 0

    def compute_direction(self, eval_x_k):  # :51-60
        direction = self.x - eval_x_k[1]
        direction = box_projection(direction, self.lb, self.ub)
        return direction - self.x

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):  # :85-108
        step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
        self.x = self.x + step * direction
        return step


class SpectralProjectedGradient(_Base):
    def __init__(self, grad_tol, x0, oracle, lower_bound, upper_bound, dot=np.dot):  # spg.rs:28-58
        self.lb, self.ub = np.asarray(lower_bound, dtype=np.float64), np.asarray(upper_bound, dtype=np.float64)
        x0 = box_projection(np.asarray(x0, dtype=np.float64), self.lb, self.ub)
        self.lambda_min, self.lambda_max = 1e-3, 1e3
        _, g0 = oracle(x0)
        direction0 = x0 - g0
        direction0 = box_projection(direction0, self.lb, self.ub)
        direction0 = direction0 - x0
        with np.errstate(divide="ignore"):
            lam = float(np.float64(1.0) / np.float64(np.max(np.abs(direction0))))
        self.lam = rmax(rmin(lam, self.lambda_max), self.lambda_min)
        self.grad_tol, self.x, self.k, self.dot = grad_tol, x0, 0, dot

    def with_lambdas(self, lambda_min, lambda_max):  # :23-27
        self.lambda_min, self.lambda_max = lambda_min, lambda_max
        return self

    def compute_direction(self, eval_x_k):  # :76-86
        direction = self.x - self.lam * eval_x_k[1]
        direction = box_projection(direction, self.lb, self.ub)
        return direction - self.x

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):  # :106-144
        step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
        xk = self.x
        next_iterate = xk + step * direction
        s_k = next_iterate - xk
        y_k = oracle(next_iterate)[1] - eval_x_k[1]
        self.x = next_iterate
        sksk = float(self.dot(s_k, s_k))
        self.last_s_norm = math.sqrt(sksk)
        skyk = float(self.dot(s_k, y_k))
        if skyk <= 0.0:
            self.lam = self.lambda_max
            return step
        self.lam = rmax(rmin(sksk / skyk, self.lambda_max), self.lambda_min)
        return step


def quadratic_fn(q, b, dot_rows=None):
    """f = 1/2 x'Qx - b'x, g = Qx - b on the host (the device objective's function)."""
    def fn(x):
        qx = q @ x
        return 0.5 * float(x @ qx) - float(b @ x), qx - b
    return fn
