"""Pure-Python (numpy float64) restatement of DESIGN.md section 34's rules 1 to 8: SpectralProximalGradient, the CPU checker of the GPU solver
QN_SPECTRAL_PROXIMAL_GRADIENT (csrc/qn_vec_prox.hip.h).  It minimises F(x) = f(x) + sum_j l1_j |x_j| over lb <= x <= ub: tests/ref_spg.py's
SpectralProjectedGradient with the projection replaced by the proximal map of lambda l1 |.| plus the box, and the two searches on composite
values with Tseng and Yun's decrease.

Element-wise numpy arithmetic on float64 rounds once per operation and never fuses a*b+c.  Every sum (g.d, h, s.s, s.y) goes through the `dot=`
parameter: numpy.dot by default, ref_spg.fsum_dot or reversed_dot for the summation-order self-check.  `faults=` plants one wrong rule by name
(tests/test_ref_prox.py shows that the comparisons reject each).  Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

from ref_spg import INF, CountingOracle, MaxIterReached, OutOfDomain, fsum_dot, rmax, rmin  # noqa: F401

FAULTS = ("tau_without_lambda", "delta_is_gd", "smooth_f_in_ring", "measure_at_zero_is_g", "h1_from_p")


def reversed_dot(a, b):
    acc = 0.0
    for v in (a * b).tolist()[::-1]:
        acc += v
    return acc


def seq_dot(a, b):
    """the products added one by one from the left, each rounded: at n <= 2 this IS the device's sum, bit for bit"""
    acc = 0.0
    for v in (a * b).tolist():
        acc += v
    return acc


def prox_direction(x, g, lam, l1, lb=None, ub=None, faults=()):
    """rule 1; returns (d, p)"""
    sg = lam * g
    u = x - sg
    tau = l1 if "tau_without_lambda" in faults else lam * l1
    z = np.where(u > tau, u - tau, np.where(u < -tau, u + tau, 0.0))
    p = z if lb is None else np.minimum(np.maximum(z, lb), ub)
    return p - x, p


def measure(x, g, l1, lb=None, ub=None, faults=()):
    """rule 2, per entry"""
    lo = np.where(x > 0.0, g + l1, g - l1)
    hi = np.where(x < 0.0, g - l1, g + l1)
    if "measure_at_zero_is_g" in faults:
        lo = np.where(x == 0.0, g, lo)
        hi = np.where(x == 0.0, g, hi)
    if lb is not None:
        lo = np.where(x == lb, -INF, lo)
        hi = np.where(x == ub, INF, hi)
    return np.where(lo > 0.0, lo, np.where(hi < 0.0, hi, 0.0))


class GLLQuadratic:
    """ref_spg.GLLQuadratic's branches on (F_t, F_k, Delta); the ring holds what the solver appends (composite values)"""

    def __init__(self, c1, m):
        self.c1, self.m, self.f_previous, self.sigma1, self.sigma2 = c1, m, [], 0.1, 0.9

    def open(self, value):
        if len(self.f_previous) == self.m:
            self.f_previous.pop(0)
        self.f_previous.append(value)
        acc = -INF
        for v in self.f_previous:
            acc = rmax(v, acc)
        self.f_max = acc

    def clear(self):
        self.f_previous = []

    def search(self, x, fk, delta, d, composite_at, max_iter):
        t, i, self.trials = 1.0, 0, 0
        while max_iter > i:
            ft = composite_at(x + t * d)
            self.trials += 1
            if ft - self.f_max <= self.c1 * t * delta:
                return t
            if t <= 0.1:
                t *= 0.5
            else:
                t_tmp = -0.5 * t * t * delta / (ft - fk - t * delta)
                if t_tmp > self.sigma1 and t_tmp < self.sigma2 * t:
                    t = t_tmp
                else:
                    t = t_tmp * 0.5
            i += 1
        return t


class BackTracking:
    def __init__(self, c1, beta):
        self.c1, self.beta = c1, beta

    def open(self, value):
        pass

    def clear(self):
        pass

    def search(self, x, fk, delta, d, composite_at, max_iter):
        t, i, self.trials = 1.0, 0, 0
        while max_iter > i:
            ft = composite_at(x + t * d)
            self.trials += 1
            if math.isnan(ft) or math.isinf(ft):
                t *= self.beta
                continue
            if ft - fk <= self.c1 * t * delta:
                return t
            t *= self.beta
            i += 1
        return t


class SpectralProximalGradient:
    def __init__(self, tol, x0, oracle, l1, lower_bound=None, upper_bound=None, dot=np.dot, faults=()):
        x0 = np.asarray(x0, dtype=np.float64)
        self.n = x0.size
        self.lb = self.ub = None
        if lower_bound is not None or upper_bound is not None:
            self.lb = np.full(self.n, -INF) if lower_bound is None else np.asarray(lower_bound, dtype=np.float64)
            self.ub = np.full(self.n, INF) if upper_bound is None else np.asarray(upper_bound, dtype=np.float64)
            x0 = np.minimum(np.maximum(x0, self.lb), self.ub)
        self.dot, self.faults = dot, tuple(faults)
        self.set_l1(l1)
        self.lambda_min, self.lambda_max = 1e-3, 1e3
        _, g0 = oracle(x0)
        d0, _ = prox_direction(x0, g0, 1.0, self.l1, self.lb, self.ub, self.faults)  # before lambda exists it counts as 1
        with np.errstate(divide="ignore"):
            lam = float(np.float64(1.0) / np.float64(np.max(np.abs(d0))))
        self.lam = rmax(rmin(lam, self.lambda_max), self.lambda_min)
        self.tol, self.x, self.k = tol, x0, 0

    def set_l1(self, v, line_search=None):
        """rule 7: the ring is cleared (it lives in the line search here), lambda and x are kept"""
        self.l1 = np.full(self.n, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64).copy()
        assert np.all(self.l1 >= 0.0) and np.all(np.isfinite(self.l1))
        if line_search is not None:
            line_search.clear()

    def with_lambdas(self, lambda_min, lambda_max):
        self.lambda_min, self.lambda_max = lambda_min, lambda_max
        return self

    def penalty(self, x=None):
        return float(self.dot(self.l1, np.abs(self.x if x is None else x)))

    def measure(self, eval_x_k):
        return measure(self.x, np.asarray(eval_x_k[1], dtype=np.float64), self.l1, self.lb, self.ub, self.faults)

    def has_converged(self, eval_x_k):
        return float(np.max(np.abs(self.measure(eval_x_k)))) < self.tol

    def minimize(self, line_search, oracle, max_iter_solver, max_iter_line_search, callback=None):
        self.k = 0
        self.trace, self.trace_x, self.trace_d, self.trace_lam = [], [], [], []
        while max_iter_solver > self.k:
            c0 = oracle.calls
            f, g = oracle(self.x)
            if math.isnan(f) or math.isinf(f):
                raise OutOfDomain()
            gnorm = float(np.max(np.abs(self.measure((f, g)))))
            if gnorm < self.tol:
                return
            lam = self.lam
            d, p = prox_direction(self.x, g, lam, self.l1, self.lb, self.ub, self.faults)
            h0 = float(self.dot(self.l1, np.abs(self.x)))
            h1 = float(self.dot(self.l1, np.abs(p if "h1_from_p" in self.faults else self.x + d)))
            gd = float(self.dot(g, d))
            delta = gd if "delta_is_gd" in self.faults else gd + (h1 - h0)
            fk = f + h0
            line_search.open(f if "smooth_f_in_ring" in self.faults else fk)
            t = line_search.search(self.x, fk, delta, d, lambda xt: oracle(xt)[0] + float(self.dot(self.l1, np.abs(xt))), max_iter_line_search)
            xn = self.x + t * d
            s = xn - self.x
            y = oracle(xn)[1] - g
            self.x = xn
            ss, sy = float(self.dot(s, s)), float(self.dot(s, y))
            self.lam = self.lambda_max if sy <= 0.0 else rmax(rmin(ss / sy, self.lambda_max), self.lambda_min)
            self.trace.append(dict(f=fk, gnorm=gnorm, t=t, n_evals=oracle.calls - c0, ls_iters=line_search.trials, s_norm=math.sqrt(ss), delta=delta))
            self.trace_x.append(self.x.copy())
            self.trace_d.append(d)
            self.trace_lam.append(lam)
            self.k += 1
            if callback is not None:
                callback(self)
        raise MaxIterReached()
