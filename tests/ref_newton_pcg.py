"""NumPy float64 restatement of the Hessian diagonal (csrc/qn_hess_diag.hip.h, slog_diag_kernel in csrc/qn_sparse_logistic.hip.h), its np.longdouble
truth with a derived entrywise bound, and the Jacobi-preconditioned inner loop of NewtonCG as a subclass of ref_newton_cg.NewtonCG.  Test
infrastructure: the product does not import this file.

THE DIAGONAL, in the device's order:
    Logistic, SparseLogistic   M_j = (sum_i d_i (a_ij a_ij)) + mu            the square rounds first; d from the weights pass at x
    LogSumExp                  M_j = ((sum_i p_i (a_ij a_ij)) - gbar_j gbar_j) + mu      the product gbar_j gbar_j rounds on its own
A row with a zero weight adds nothing.  (The dense kernel accumulates with an FMA and the sum's order is the device's cut: both lie inside the bound
below, which holds for any order, with or without FMA.)

THE BOUNDS are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u), S_j = sum_i d*_i a_ij^2 (every term non-negative).
    logistic pair   |M_j - M*_j| <= sum_i a_ij^2 bd_i + gamma_(rows + 3) S_j + u (S_j + |mu|)
                    bd_i: ref_logistic.truth_and_bound's bound on d_i; `rows + 3`: the square, the product, rows - 1 additions in any order and the
                    addition of mu (rows = m for a dense A, at most m for a column of a sparse one); u (S_j + |mu|): the last addition's result.
    log-sum-exp     p_i carries the relative error eta and gbar_j the error (m u + eta) G_j, G_j = sum_i p_i |a_ij| >= |gbar_j|, with
                    B = (2 m + 4 (n + 1) Z + 16) u >= eta + m u (lse_hess_vec_cases, step (1)).  S_j: (eta + (m + 3) u) S_j <= (B + 3 u) S_j;
                    gbar_j^2: 2 |gbar_j| B G_j + u gbar_j^2 <= (2 B + u) G_j^2; the subtraction and the addition: 2 u (S_j + G_j^2 + |mu|).
                    |M_j - M*_j| <= (B + 5 u) S_j + (2 B + 3 u) G_j^2 + 2 u |mu|.
The longdouble reference's own error -- the same expressions with 2^-64 for u, a factor 2^-11 -- is added.

ONE PRECONDITIONED DIRECTION (rules 2', 5', 7' of csrc/qn_newton_cg.hip.h; 1, 3, 4, 6, 8 are ref_newton_cg's):
    1'. M = diag H(x) by `diag_at(x)` after the weights at x, once per direction
    2'. minv_j = 1 / M_j when M_j > 0 and finite, else 1 (counted in `floored`); z = 0, r = g, p = minv o g, gg = g.g,
        rz = sum r_j (minv_j r_j) (the inner product rounds first); eta as rule 2
    5'. alpha = rz / kappa; z += alpha p, r -= alpha q; rr' = r.r, rz' = r.(minv o r), g.z
    6.  sqrt(rr') <= eta sqrt(gg) on the EUCLIDEAN residual, unchanged
    7'. beta = rz' / rz; p = minv o r + beta p (both products round first); rz = rz'"""
import math

import numpy as np

import lse_hess_vec_cases as HV
import ref_logistic as RL
import ref_newton_cg as RN

U = 2.0 ** -53
LD = np.longdouble
REF = 1.0 + 2.0 ** -11


def _cols(sq, w, dot):
    return sq.T @ w if dot is None else np.array([dot(col, w) for col in np.ascontiguousarray(sq.T)])


def logistic_diag_at(a, y, w, mu, dot=None):
    """x -> diag H(x) of the logistic pair in float64 (a sparse A: its densified matrix -- an absent entry adds an exact zero)"""
    sq = a * a

    def at_x(x):
        return _cols(sq, RL.weights_f64(a, y, w, x, dot), dot) + mu
    return at_x


def lse_diag_at(a, c, mu, dot=None):
    """x -> diag H(x) of log-sum-exp in float64: (sum_i p_i a_ij^2 - gbar_j gbar_j) + mu"""
    sq = a * a

    def at_x(x):
        z = a @ x + c
        e = np.exp(z - z.max())
        p = e / e.sum()
        gbar = _cols(a, p, dot)
        return (_cols(sq, p, dot) - gbar * gbar) + mu
    return at_x


def logistic_diag_truth(a, y, w, mu, x, truth=None):
    """(M* in longdouble, its entrywise bound in longdouble); `truth`: ref_logistic.truth_and_bound at x where the caller has it"""
    truth = truth or RL.truth_and_bound(a, y, w, mu, x)
    sq = a.astype(LD) ** 2
    s = sq.T @ truth["d"]
    rows = np.count_nonzero(a, axis=0)  # (a dense Gaussian A: m; a sparse one: the column's entries)
    gam = np.array([RL.gamma(int(r) + 3) for r in rows]).astype(LD)
    bound = sq.T @ truth["bd"] + gam * s + LD(U) * (s + abs(LD(mu)))
    return s + LD(mu), bound * LD(REF)


def lse_diag_truth(a, c, mu, x):
    """(M* in longdouble, its entrywise bound in longdouble) of log-sum-exp; a masked row (c = -inf) has p = 0 exactly and enters nothing"""
    m, n = a.shape
    al, p, gbar = HV.weights(a, c, x)
    s = (al ** 2).T @ p
    g_abs = np.abs(al).T @ p
    live = np.isfinite(c)
    zcap = float(np.max(np.abs(a[live]) @ np.abs(x) + np.abs(c[live])))
    b = (2 * m + 4 * (n + 1) * zcap + 16) * U
    bound = LD(b + 5 * U) * s + LD(2 * b + 3 * U) * g_abs ** 2 + LD(2 * U) * abs(LD(mu))
    return (s - gbar * gbar) + LD(mu), bound * LD(REF)


def ratio(got, truth, bound):
    """the largest |error| / bound; a zero bound with a zero error counts as 0, a non-finite value is never inside a bound"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    return float(np.max(np.where(np.isnan(r), LD(np.inf), r)))


def minv_of(m):
    """rule 2': (minv, the number of substituted entries)"""
    ok = (m > 0.0) & np.isfinite(m)
    with np.errstate(all="ignore"):
        return np.where(ok, 1.0 / np.where(ok, m, 1.0), 1.0), int(np.count_nonzero(~ok))


class JacobiNewtonCG(RN.NewtonCG):
    """ref_newton_cg.NewtonCG with the Jacobi preconditioner.  `diag_at`: x -> diag H(x).  twice=True plants the fault `minv applied twice`."""

    def __init__(self, tol, x0, hess_vec_at, diag_at, eta_max=0.5, max_inner=0, dot=np.dot, twice=False):
        super().__init__(tol, x0, hess_vec_at, eta_max=eta_max, max_inner=max_inner, dot=dot)
        self.diag_at, self.twice = diag_at, twice
        self.diag_passes, self.floored = 0, []

    def compute_direction(self, eval_x_k):
        g, dot = eval_x_k[1], self.dot
        hv = self.hess_vec_at(self.x)
        minv, floored = minv_of(self.diag_at(self.x))
        if self.twice:
            minv = minv * minv
        self.diag_passes += 1
        self.floored.append(floored)
        z, r, p = np.zeros_like(g), g.copy(), minv * g
        gg = float(dot(g, g))
        rz, j = float(dot(r, minv * r)), 0
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
            alpha = RN._div(rz, kappa)
            z = z + alpha * p
            r = r - alpha * q
            j += 1
            y = minv * r
            rrn, rzn, gz = float(dot(r, r)), float(dot(r, y)), float(dot(g, z))
            rz_old, rz = rz, rzn
            if math.sqrt(rrn) <= eta * sqgg:
                why = "tol"
                break
            if j >= self.cap:
                why = "cap"
                break
            beta = RN._div(rzn, rz_old)
            p = y + beta * p
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
