"""NumPy float64 restatement of the device logistic objective (csrc/qn_logistic.hip.h) in the device's association, and its np.longdouble truth with
derived bounds.  Test infrastructure: the product does not import this file.

    f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2,   g = -A'(y o w o s) + mu x,   H = A' diag(d) A + mu I

THE DEVICE'S ORDER, per row:  z = sign(yw) (a_r . x);  t = |z|;  e = exp(-t);  q = 1 + e;  s = z >= 0 ? e / q : 1 / q;
l = |yw| (max(-z, 0) + log1p(e));  coefficient = -(yw s);  d = |yw| ((e / q) / q);  yw = 0: l = coefficient = d = 0.

THE BOUNDS are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u), zeta_r = sum_j |a_rj| |x_j|, dz_r = gamma_(n+2) zeta_r (the dot in any
order, with or without FMA), C = 8 (a cap on the exp / log1p / division chains in ulp, not a measurement):

    |f - f*|     <= sum_r w_r (s_r dz_r + C u l_r) + gamma_(m+2) sum_r w_r l_r + gamma_(n+3) |mu|/2 ||x||^2 + u |f*|        (|dl/dz| = s)
    |g_j - g*_j| <= sum_r |a_rj| w_r (dz_r / 4 + C u s_r) + gamma_(m+2) sum_r |a_rj| w_r s_r + 2 u |mu x_j| + u |g*_j|      (|ds/dz| <= 1/4)
    |d_r - d*_r| <= w_r (0.0963 dz_r + C u d*_r)                                         (0.0963 >= max |s (1 - s)(1 - 2 s)| = 1 / (6 sqrt 3))
    |q_j - q*_j| <= sum_r |a_rj| (E(d_r) U_r + (gamma_(n+1) + gamma_(m+2) + u) d_r U_r) + 3 u |mu v_j|,   U_r = sum_j |a_rj| |v_j|
    |c - c*|     <= sum_j |v_j| E(q_j) + gamma_(n+2) sum_j |v_j q*_j|                                   (tests/lse_hess_vec_cases.py's pattern)

(s_r, l_r, d_r without weights on the right-hand sides.)  The product's bound is lse_hess_vec_cases.truth_and_bound's with the gbar terms dropped and
d's bound propagated.  The longdouble reference's own error -- the same expressions with 2^-64 for u, a factor 2^-11 -- is added."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
C_ULP = 8.0
REF = 1.0 + 2.0 ** -11


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


def row_terms(yw, u):
    """(l, coefficient, d, s) of every row from its label-and-weight yw and its dot u = a_r . x, in the device's order"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        z = np.where(yw < 0.0, -u, u)
        t = np.abs(z)
        e = np.exp(-t)
        q = 1.0 + e
        s = np.where(z >= 0.0, e, 1.0) / q
        aw = np.abs(yw)
        l = aw * (np.maximum(-z, 0.0) + np.log1p(e))
        coef = -(yw * s)
        d = aw * ((e / q) / q)
    live = yw != 0.0
    return np.where(live, l, 0.0), np.where(live, coef, 0.0), np.where(live, d, 0.0), s


def _matvec(mat, x, dot):
    return mat @ x if dot is None else np.array([dot(row, x) for row in mat])


def logistic_fn(a, y, w, mu, dot=None):
    """x -> (f, g) in float64; `dot`: the summation order of every inner product (None: numpy's matrix products)"""
    yw = np.asarray(y, dtype=np.float64) * (np.ones(len(y)) if w is None else np.asarray(w, dtype=np.float64))
    at = np.ascontiguousarray(a.T)
    ones = np.ones(a.shape[0])

    def fn(x):
        l, coef, _, _ = row_terms(yw, _matvec(a, x, dot))
        xx = float(x @ x) if dot is None else float(dot(x, x))
        fsum = float(np.sum(l)) if dot is None else float(dot(l, ones))
        return fsum + 0.5 * mu * xx, _matvec(at, coef, dot) + mu * x
    return fn


def logistic_hess_vec_at(a, y, w, mu, dot=None):
    """x -> (v -> H(x) v) in the device's association: A'(d o (A v)) + mu v, each w_r = d_r u_r rounded once"""
    yw = np.asarray(y, dtype=np.float64) * (np.ones(len(y)) if w is None else np.asarray(w, dtype=np.float64))
    at = np.ascontiguousarray(a.T)

    def at_x(x):
        d = row_terms(yw, _matvec(a, x, dot))[2]

        def hv(v):
            return _matvec(at, d * _matvec(a, v, dot), dot) + mu * v
        return hv
    return at_x


def weights_f64(a, y, w, x, dot=None):
    yw = np.asarray(y, dtype=np.float64) * (np.ones(len(y)) if w is None else np.asarray(w, dtype=np.float64))
    return row_terms(yw, _matvec(a, x, dot))[2]


def truth_and_bound(a, y, w, mu, x, v=None):
    """dict: f, g, d (and q, c for a v) in longdouble with their bounds (bf, bg, bd, bq, bc) in longdouble, the reference's share included"""
    m, n = a.shape
    w = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    al, xl, yl, wl = a.astype(LD), x.astype(LD), np.asarray(y).astype(LD), w.astype(LD)
    z = yl * (al @ xl)
    t = np.abs(z)
    e = np.exp(-t)
    q = 1 + e
    s = np.where(z >= 0, e / q, 1 / q)
    l = np.maximum(-z, 0) + np.log1p(e)
    d1 = (e / q) / q  # s (1 - s) without the cancellation
    f = np.sum(wl * l) + LD(mu) / 2 * (xl @ xl)
    g = -(al.T @ (yl * wl * s)) + LD(mu) * xl
    d = wl * d1
    aa, ax = np.abs(a).astype(LD), np.abs(x).astype(LD)
    dz = LD(gamma(n + 2)) * (aa @ ax)
    cu = LD(C_ULP * U)
    bf = np.sum(wl * (s * dz + cu * l)) + LD(gamma(m + 2)) * np.sum(wl * l) + LD(gamma(n + 3)) * abs(LD(mu)) / 2 * (xl @ xl) + LD(U) * abs(f)
    bg = aa.T @ (wl * (dz / 4 + cu * s)) + LD(gamma(m + 2)) * (aa.T @ (wl * s)) + 2 * LD(U) * np.abs(LD(mu) * xl) + LD(U) * np.abs(g)
    bd = wl * (LD(0.0963) * dz + cu * d1)
    out = dict(f=f, g=g, d=d, s=s, bf=bf * LD(REF), bg=bg * LD(REF), bd=bd * LD(REF))
    if v is not None:
        vl, av = v.astype(LD), np.abs(v).astype(LD)
        qv = al.T @ (d * (al @ vl)) + LD(mu) * vl
        uk = aa @ av
        bq = aa.T @ (bd * uk + LD(gamma(n + 1) + gamma(m + 2) + U) * (d * uk)) + 3 * LD(U) * np.abs(LD(mu) * vl)
        bq = bq * LD(REF)
        bc = np.sum(av * bq) + LD(gamma(n + 2) * REF) * np.sum(av * np.abs(qv))
        out.update(q=qv, c=vl @ qv, bq=bq, bc=bc)
    return out


def ratios(got, truth):
    """the largest |error| / bound per quantity in `got` (f, g, d, q, c as available); a zero bound with a zero error counts as 0"""
    out = {}
    for key, bkey in (("f", "bf"), ("g", "bg"), ("d", "bd"), ("q", "bq"), ("c", "bc")):
        if key not in got or key not in truth:
            continue
        err = np.abs(np.asarray(got[key], dtype=np.float64).astype(LD) - truth[key])
        bound = np.asarray(truth[bkey], dtype=LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, LD(0), err / bound)
        r = np.where(np.isnan(r), LD(np.inf), r)  # (a non-finite value is never inside a bound)
        out[key] = float(np.max(r))
    return out
