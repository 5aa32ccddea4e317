"""NumPy float64 restatement of the device multinomial objective (csrc/qn_multinomial.hip.h) in the device's association, and its np.longdouble truth
with derived bounds.  Test infrastructure: the product does not import this file.

The parameter vector is class-major, x[k n + j] = W[k, j].  With z_rk = a_r . W_k and p_r = softmax_k(z_r):

    f = sum_r w_r (logsumexp_k z_rk - z_{r,y_r}) + mu/2 ||x||^2,   g_k = sum_r c_rk a_r + mu W_k,   (H v)_k = sum_r t_rk a_r + mu V_k

THE DEVICE'S ORDER, per row:  zmax = max_k z_k;  e_k = exp(z_k - zmax);  S = sum_k e_k in class order;  p_k = e_k / S;  l = (zmax - z_y) + log(S);
c_k = w p_k (k != y),  c_y = -(w (Sn / S)) with Sn = sum_{k != y} e_k in class order;  the stored P_k = p_k;  w = 0: l = c_k = P_k = 0.
Product: u_k = a_r . V_k,  ubar = sum_k P_k u_k in class order,  t_k = (w P_k)(u_k - ubar);  w = 0: t_k = 0.

THE BOUNDS are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u), C = 8 (ref_logistic's cap on the exp / log / division chains in ulp).
  The margins.  dz_r = gamma_(n+2) max_k sum_j |a_rj| |W_kj| bounds every computed margin's error (a dot in any order, with or without FMA).  The
  exponent z_k - zmax is rounded once more: u |z_k - zmax| <= u spread_r.  eps_r = dz_r + u spread_r is the perturbation of the margins the row sees.
  The loss.  logsumexp is 1-Lipschitz in the maximum norm, so |dl| <= 2 eps_r EXACTLY (no second-order remainder).  Its roundings: S carries the
  relative error gamma_K + C u of K exp's summed, so log(S) an ABSOLUTE error gamma_K + C u, plus C u log(S), plus u for each of the two adds:
      |l - l*| <= 2 eps_r + (gamma_(K+1) + 2 C u)(1 + l*_r)
  (the absolute part is the price of the rule l = (zmax - z_y) + log(S): where the row is fitted l is small and log(S) = log(1 + tiny)).
  The probabilities.  p_k(z + d) / p_k(z) = e^{d_k} / sum_j p_j e^{d_j} lies in [e^{-2 eps}, e^{2 eps}]: |dp_k| <= p_k expm1(2 eps_r), which is
  2 p_k eps_r and its whole remainder (for 2 eps_r <= 1 it is below 2 p_k eps_r (1 + 2 eps_r)).  Roundings: exp (C u), S and Sn (gamma_K each), the
  division (u):
      rho_r = expm1(2 eps_r) + gamma_(2K+2) + 2 C u,      |p_k - p*_k| <= rho_r p*_k
  The coefficients.  |c_k - c*_k| <= (rho_r + 2 u) |c*_k| for every k -- for the labelled class |c*_y| = w (1 - p_y) = w sum_{k != y} p_k, each term with
  the relative error rho_r: the error is C u (1 - p_y), not u, which is why the device never forms p_y - 1.
      |f - f*|       <= sum_r w_r (2 eps_r + (gamma_(K+1) + 2 C u)(1 + l*_r)) + gamma_(m+2) sum_r w_r l*_r + gamma_(N+3) |mu|/2 ||x||^2 + u |f*|
      |g_kj - g*_kj| <= sum_r |a_rj| |c*_rk| (rho_r + 2 u + gamma_(m+2)) + 2 u |mu x_kj| + u |g*_kj|
  The product.  eta_r = gamma_(n+2) max_k sum_j |a_rj| |V_kj| bounds the error of u_k; Ubar_r = sum_k p_k |u_k|:
      |ubar - ubar*| <= (rho_r + gamma_(K+1)) Ubar_r + eta_r
      |t_k - t*_k|   <= w p_k (rho_r |u_k - ubar| + 2 eta_r + (rho_r + gamma_(K+1)) Ubar_r + 3 u (|u_k| + |ubar|))            =: E(t_rk)
      |q_kj - q*_kj| <= sum_r |a_rj| (E(t_rk) + (gamma_(m+2) + u) |t*_rk|) + 3 u |mu v_kj|
      |c - c*|       <= sum |v| E(q) + gamma_(N+2) sum |v q*|                                           (ref_logistic's bq, bc)
  (products of two first-order terms are left to the reference's share; every p_k, c_k and t_k also gets float64's underflow step 2^-1074, which
  matters only where e_k underflows: at a spread of 1600 the device's p_k is exactly 0 and the truth's is 1e-695.)  The longdouble reference's own error -- the same expressions with 2^-64 for
  u, a factor 2^-11 -- is added: REF = 1 + 2^-11."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
C_ULP = 8.0
REF = 1.0 + 2.0 ** -11
UF = 2.0 ** -1074  # float64's smallest step near zero: an e_k (and with it p_k, c_k) that underflows is off by at most this, whatever rho says


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


def _matmul(a, b, dot):
    """a (p x q) times b (q x r) with every inner product by `dot` (None: numpy's product)"""
    if dot is None:
        with np.errstate(over="ignore", invalid="ignore"):  # (a masked row's margins may overflow: row_terms selects them away)
            return a @ b
    bt = np.ascontiguousarray(b.T)
    return np.array([[dot(row, col) for col in bt] for row in a]).reshape(a.shape[0], b.shape[1])


def row_terms(z, y, w):
    """(l, c, P) of every row from its margins z (m x K), in the device's order"""
    m, k = z.shape
    rows = np.arange(m)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        zmax = np.max(z, axis=1)
        e = np.exp(z - zmax[:, None])
        s = np.zeros(m)
        sn = np.zeros(m)
        for j in range(k):  # class order, plain adds
            s = s + e[:, j]
            sn = sn + np.where(y == j, 0.0, e[:, j])
        p = e / s[:, None]
        l = w * ((zmax - z[rows, y]) + np.log(s))
        c = w[:, None] * p
        c[rows, y] = -(w * (sn / s))
    live = w != 0.0
    return np.where(live, l, 0.0), np.where(live[:, None], c, 0.0), np.where(live[:, None], p, 0.0)


def _prep(a, y, w):
    y = np.asarray(y).astype(np.int64)
    w = np.ones(a.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    return y, w


def multinomial_fn(a, y, w, k, mu, dot=None):
    """x -> (f, g) in float64, x and g class-major; `dot`: the summation order of every inner product (None: numpy's matrix products)"""
    y, w = _prep(a, y, w)
    m, n = a.shape
    ones = np.ones(m)

    def fn(x):
        wm = x.reshape(k, n)
        l, c, _ = row_terms(_matmul(a, wm.T, dot), y, w)
        xx = float(x @ x) if dot is None else float(dot(x, x))
        fsum = float(np.sum(l)) if dot is None else float(dot(l, ones))
        return fsum + 0.5 * mu * xx, (_matmul(c.T, a, dot) + mu * wm).ravel()
    return fn


def probabilities_f64(a, y, w, k, x, dot=None):
    y, w = _prep(a, y, w)
    return row_terms(_matmul(a, x.reshape(k, a.shape[1]).T, dot), y, w)[2]


def multinomial_hess_vec_at(a, y, w, k, mu, dot=None):
    """x -> (v -> H(x) v) in the device's association"""
    y, w = _prep(a, y, w)
    n = a.shape[1]

    def at_x(x):
        p = probabilities_f64(a, y, w, k, x, dot)

        def hv(v):
            vm = v.reshape(k, n)
            with np.errstate(over="ignore", invalid="ignore"):
                u = _matmul(a, vm.T, dot)
                ub = np.zeros(a.shape[0])
                for j in range(k):  # class order
                    ub = ub + p[:, j] * u[:, j]
                t = (w[:, None] * p) * (u - ub[:, None])
            t = np.where((w != 0.0)[:, None], t, 0.0)
            return (_matmul(t.T, a, dot) + mu * vm).ravel()
        return hv
    return at_x


def truth_and_bound(a, y, w, k, mu, x, v=None):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        return _truth_and_bound(a, y, w, k, mu, x, v)


def _truth_and_bound(a, y, w, k, mu, x, v):
    """dict: f, g, p (m x K; masked rows zero) and, for a v, q and c in longdouble with their bounds bf, bg, bp, bq, bc (the reference's share included)"""
    y, w = _prep(a, y, w)
    m, n = a.shape
    nn = k * n
    rows = np.arange(m)
    al, wl, xl = a.astype(LD), w.astype(LD), x.astype(LD)
    wm = xl.reshape(k, n)
    z = al @ wm.T
    zmax = np.max(z, axis=1)
    e = np.exp(z - zmax[:, None])
    s = np.sum(e, axis=1)
    p = e / s[:, None]
    l = (zmax - z[rows, y]) + np.log(s)
    onehot = np.zeros((m, k), dtype=LD)
    onehot[rows, y] = 1
    c = wl[:, None] * p
    c[rows, y] = -(wl * (np.sum(np.where(onehot == 1, 0, e), axis=1) / s))  # w (p_y - 1) without the cancellation
    live = (w != 0.0)
    l, c = np.where(live, l, LD(0)), np.where(live[:, None], c, LD(0))  # (a masked row's margins may not be finite)
    f = np.sum(wl * l) + LD(mu) / 2 * (xl @ xl)
    g = (c.T @ al + LD(mu) * wm).ravel()
    aa = np.abs(a).astype(LD)
    dz = LD(gamma(n + 2)) * np.max(aa @ np.abs(wm).T, axis=1)
    eps = dz + LD(U) * (zmax - np.min(z, axis=1))
    eps = np.where(live, eps, LD(0))
    cu = LD(C_ULP * U)
    rho = np.expm1(2 * eps) + LD(gamma(2 * k + 2)) + 2 * cu
    bf = (np.sum(wl * (2 * eps + (LD(gamma(k + 1)) + 2 * cu) * (1 + l))) + LD(gamma(m + 2)) * np.sum(wl * l)
          + LD(gamma(nn + 3)) * abs(LD(mu)) / 2 * (xl @ xl) + LD(U) * abs(f))
    ac = np.abs(c)
    bg = ((ac * (rho + 2 * LD(U) + LD(gamma(m + 2)))[:, None] + wl[:, None] * LD(UF)).T @ aa).ravel() + 2 * LD(U) * np.abs(LD(mu) * xl) + LD(U) * np.abs(g)
    pm = np.where(live[:, None], p, LD(0))
    bp = np.where(live[:, None], rho[:, None] * p + LD(UF), LD(0))
    out = dict(f=f, g=g, p=pm, l=l, bf=bf * LD(REF), bg=bg * LD(REF), bp=bp * LD(REF))
    if v is not None:
        vl = v.astype(LD)
        vm = vl.reshape(k, n)
        u = al @ vm.T
        ub = np.sum(p * u, axis=1)
        t = np.where(live[:, None], (wl[:, None] * p) * (u - ub[:, None]), LD(0))
        q = (t.T @ al + LD(mu) * vm).ravel()
        eta = LD(gamma(n + 2)) * np.max(aa @ np.abs(vm).T, axis=1)
        ubar_abs = np.sum(p * np.abs(u), axis=1)
        bt = (wl[:, None] * p) * (rho[:, None] * np.abs(u - ub[:, None]) + (2 * eta + (rho + LD(gamma(k + 1))) * ubar_abs)[:, None]
                                  + 3 * LD(U) * (np.abs(u) + np.abs(ub)[:, None])) + wl[:, None] * LD(UF) * np.abs(u - ub[:, None])
        bt = np.where(live[:, None], bt, LD(0))
        bq = ((bt + LD(gamma(m + 2) + U) * np.abs(t)).T @ aa).ravel() + 3 * LD(U) * np.abs(LD(mu) * vl)
        bq = bq * LD(REF)
        av = np.abs(vl)
        bc = np.sum(av * bq) + LD(gamma(nn + 2) * REF) * np.sum(av * np.abs(q))
        out.update(q=q, c=vl @ q, bq=bq, bc=bc)
    return out


def ratios(got, truth):
    """the largest |error| / bound per quantity in `got` (f, g, p, q, c as available); a zero bound with a zero error counts as 0"""
    out = {}
    for key, bkey in (("f", "bf"), ("g", "bg"), ("p", "bp"), ("q", "bq"), ("c", "bc")):
        if key not in got or key not in truth:
            continue
        err = np.abs(np.asarray(got[key], dtype=np.float64).astype(LD) - truth[key])
        bound = np.asarray(truth[bkey], dtype=LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, LD(0), err / bound)
        r = np.where(np.isnan(r), LD(np.inf), r)  # (a non-finite value is never inside a bound)
        out[key] = float(np.max(r))
    return out
