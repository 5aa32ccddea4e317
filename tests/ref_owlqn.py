"""Pure-Python (numpy float64) restatement of DESIGN.md section 35's rules 1 to 9: OWLQN, the CPU checker of the GPU solver QN_OWLQN
(csrc/qn_vec_owlqn.hip.h), on the machine of tests/ref_lbfgs.py and tests/ref_spg.py.  It minimises F(x) = f(x) + sum_j l1_j |x_j| without a box
by orthant-wise limited-memory quasi-Newton (Andrew and Gao, ICML 2007).

z = H_k v comes from the TWO-LOOP RECURSION by default -- not the compact form the GPU kernels use --; `direction="compact"` is the compact form
for the self-checks.  Element-wise numpy arithmetic on float64 rounds once per operation and never fuses a*b+c.  Every sum (v.z, v.d, h,
v.(xt - x), s.s, s.y, y.y) goes through the `dot=` parameter: numpy.dot by default, ref_spg.fsum_dot or ref_prox.reversed_dot for the
summation-order self-check, ref_prox.seq_dot at n <= 2.  `faults=` plants one wrong rule by name (tests/test_ref_owlqn.py shows that the
comparisons reject each).  Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

import ref_lbfgs as RL
import ref_prox as RP
from ref_spg import CountingOracle, MaxIterReached, OutOfDomain  # noqa: F401

FAULTS = ("pg_at_zero_is_g", "no_alignment", "orthant_from_x", "accept_unprojected", "y_from_pseudo", "armijo_t_vd", "no_exemption")


class AbnormalTermination(Exception):
    pass


def pseudo_gradient(x, g, l1, faults=()):
    """rule 1: ref_prox.measure without a box"""
    v = RP.measure(x, g, l1)
    if "pg_at_zero_is_g" in faults:
        v = np.where(x == 0.0, g, v)
    return v


def align(z, v, l1, faults=()):
    """rule 3: d = -z where the entry is smooth or z and v have one strict sign, else the literal 0.0"""
    keep = ((z > 0.0) & (v > 0.0)) | ((z < 0.0) & (v < 0.0))
    if "no_exemption" not in faults:
        keep = keep | (l1 == 0.0)
    if "no_alignment" in faults:
        keep = np.ones_like(keep)
    return np.where(keep, -z, 0.0)


def project(x, d, v, l1, t, faults=()):
    """rules 4 and 5: u = x + t d (t d rounded first), kept where the entry is smooth or u has xi's strict sign"""
    u = x + t * d
    if "orthant_from_x" in faults:
        pos, neg = x > 0.0, x < 0.0
    else:
        pos, neg = (x > 0.0) | ((x == 0.0) & (v < 0.0)), (x < 0.0) | ((x == 0.0) & (v > 0.0))
    keep = ((u > 0.0) & pos) | ((u < 0.0) & neg)
    if "no_exemption" not in faults:
        keep = keep | (l1 == 0.0)
    return np.where(keep, u, 0.0)


class BackTracking:
    """the one search OWLQN takes: only its two numbers are used, the loop is the solver's (rule 6)"""

    def __init__(self, c1, beta):
        self.c1, self.beta = c1, beta


class OWLQN:
    def __init__(self, tol, x0, l1, m=5, unit_scaling=False, dot=np.dot, direction="two_loop", faults=()):
        self.x = np.array(x0, dtype=np.float64)
        self.n = self.x.size
        self.tol, self.k, self.m, self.unit, self.dot, self.faults = tol, 0, m, unit_scaling, dot, tuple(faults)
        self.hv = {"two_loop": RL.two_loop, "compact": RL.compact}[direction]
        self.pairs, self.resets, self.gamma, self.updated = [], 0, 1.0, []
        self.set_l1(l1)

    def set_l1(self, v):
        """rule 9: the pairs, x (and the memo) are kept"""
        self.l1 = np.full(self.n, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64).copy()
        assert np.all(self.l1 >= 0.0) and np.all(np.isfinite(self.l1))

    def set_memory(self, m):
        self.m, self.pairs, self.gamma = m, [], 1.0

    def stored_pairs(self):
        return len(self.pairs)

    def penalty(self, x=None):
        return float(self.dot(self.l1, np.abs(self.x if x is None else x)))

    def measure(self, eval_x_k):
        return pseudo_gradient(self.x, np.asarray(eval_x_k[1], dtype=np.float64), self.l1, self.faults)

    def has_converged(self, eval_x_k):
        return float(np.max(np.abs(self.measure(eval_x_k)))) < self.tol

    def hk(self, v):
        """rule 2: z = H_k v with QN_LBFGS's safeguard on v.z"""
        z = v
        if self.pairs:
            s, y = self.pairs[-1]
            with np.errstate(all="ignore"):
                self.gamma = 1.0 if self.unit else float(self.dot(s, y)) / float(self.dot(y, y))
                z = self.hv(self.pairs, v, self.gamma, self.dot)
                vz = float(self.dot(v, z))
            if not (vz > 0.0) or math.isinf(vz):
                self.pairs, self.resets, self.gamma, z = [], self.resets + 1, 1.0, v
        else:
            self.gamma = 1.0
        return z

    def minimize(self, line_search, oracle, max_iter_solver, max_iter_line_search, callback=None):
        self.k = 0
        self.trace, self.trace_x, self.trace_d, self.trace_v, self.trace_z, self.updated = [], [], [], [], [], []
        c1, beta, faults, dot = line_search.c1, line_search.beta, self.faults, self.dot
        while max_iter_solver > self.k:
            c0 = oracle.calls
            f, g = oracle(self.x)
            if math.isnan(f) or math.isinf(f):
                raise OutOfDomain()
            x, l1 = self.x, self.l1
            v = pseudo_gradient(x, g, l1, faults)
            gnorm = float(np.max(np.abs(v)))
            if gnorm < self.tol:
                return
            z = self.hk(v)
            d = align(z, v, l1, faults)
            vd = float(dot(v, d))
            if not (vd < 0.0) or math.isinf(vd):
                raise AbnormalTermination("not a descent direction")
            fk = f + float(dot(l1, np.abs(x)))
            t, i, trials = 1.0, 0, 0
            while max_iter_line_search > i:
                xt = project(x, d, v, l1, t, faults)
                ft = oracle(xt)[0] + float(dot(l1, np.abs(xt)))
                trials += 1
                if math.isnan(ft) or math.isinf(ft):
                    t *= beta
                    continue
                rhs = c1 * t * vd if "armijo_t_vd" in faults else c1 * float(dot(v, xt - x))
                if ft - fk <= rhs:
                    break
                t *= beta
                i += 1
            xn = x + t * d if "accept_unprojected" in faults else project(x, d, v, l1, t, faults)
            gn = oracle(xn)[1]
            s = xn - x
            y = pseudo_gradient(xn, gn, l1, faults) - v if "y_from_pseudo" in faults else gn - g
            self.x = xn
            ss, sy, yy = float(dot(s, s)), float(dot(s, y)), float(dot(y, y))
            commit = sy > RL.EPS * yy
            if commit:
                self.pairs.append((s, y))
                if len(self.pairs) > self.m:
                    self.pairs.pop(0)
            self.updated.append(1 if commit else 0)
            self.trace.append(dict(f=fk, gnorm=gnorm, t=t, n_evals=oracle.calls - c0, ls_iters=trials, s_norm=math.sqrt(ss), vd=vd, updated=int(commit)))
            self.trace_x.append(xn.copy())
            self.trace_d.append(d)
            self.trace_v.append(v)
            self.trace_z.append(z)
            self.k += 1
            if callback is not None:
                callback(self)
        raise MaxIterReached()
