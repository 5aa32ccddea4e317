"""What tests/test_ref_lse_hess_vec.py (CPU) and tests/test_gpu_lse_hess_vec.py (GPU) share: the log-sum-exp Hessian-vector product
q = H(x) v = A'(p o (A v)) - gbar (p . (A v)) + mu v (qn_objective_hess_vec_at, csrc/qn_lse_hv.hip.h) in np.longdouble, and its derived
element-wise error bound.  numpy only; the problems are spg_cases.lse_problem's, as in newton_lse_cases.py.

THE BOUND is derived, not measured; nothing in it comes from the code under test.  With u = 2^-53, p = softmax(A x + c), U_k = sum_j |a_kj| |v_j|,
G_i = sum_k p_k |a_ki|, S^C_ij = sum_k p_k |a_ki| |a_kj|, S = S^C + G G' + mu I (the scale matrix of newton_lse_cases.hessian_truth_and_bound),
Z = max_k (sum_j |a_kj x_j| + |c_k|) over the rows that are not masked, and to first order in u:

    (1) p_k carries the relative error eta <= (4 (n + 1) Z + m + c1) u and gbar_i the error (m u + eta) G_i: DESIGN.md 20, steps (1), (2), (4).
        A masked row (c_k = -inf) has p_k = 0 exactly, on the device and in the truth: it enters no sum and not Z.
    (2) u_k = a_k . v is an n-term sum in any order, with or without FMA: |du_k| <= n u U_k.
    (3) w_k = p_k u_k, one rounding: |dw_k| <= (eta + (n + 1) u) p_k U_k.
    (4) sum_k w_k a_kj is an m-term sum in any order (FMA chains per workgroup, then the workgroups' results added): m u sum_k |w_k| |a_kj|, plus
        (3) through the terms: (eta + (n + m + 1) u) sum_k p_k U_k |a_kj| = (eta + (n + m + 1) u) (S^C |v|)_j.
    (5) ubar = sum_k w_k likewise: (eta + (n + m + 1) u) sum_k p_k U_k = (eta + (n + m + 1) u) (G . |v|), and |ubar| <= G . |v|.
    (6) the product ubar gbar_j: |ubar| |dgbar_j| + |dubar| |gbar_j| + u |ubar gbar_j| <= (2 eta + (2 m + n + 2) u) G_j (G . |v|)
        = (2 eta + (2 m + n + 2) u) (G G' |v|)_j.
    (7) mu v_j: u mu |v_j|; the subtraction and the addition: 2 u (S |v|)_j at the most.
    Sum: |q_j - q*_j| <= (eta + (n + m + 3) u) (S^C |v|)_j + (2 eta + (2 m + n + 4) u) (G G' |v|)_j + 3 u mu |v_j|.

newton_lse_cases' constant is B = (2 m + 4 (n + 1) Z + 16) u >= eta + m u (c1 <= 16, as there), so 2 B >= 2 eta + 2 m u and every coefficient above
is at most

    B_v = 2 B + (n + 4) u,          |q_j - q*_j| <= B_v (S |v|)_j.

(S |v|)_j is formed without the matrix: sum_k p_k |a_kj| U_k + G_j (G . |v|) + mu |v_j|.

v'Hv is a sum of n products v_j q_j of the COMPUTED q_j, in shares, any order: tests/hess_vec_cases.py's pattern,
    |c - c*| <= sum_j |v_j| E(q_j) + gamma_(n + 2) sum_j |v_j q*_j|,     E(q_j) = B_v (S |v|)_j.

The reference is np.longdouble (u = 2^-64): its own error, the same expressions with 2^-64 for u (a factor 2^-11), is added; comparisons are made
in longdouble, so the truth is never rounded to float64."""
import functools

import numpy as np

import newton_lse_cases as NL

U = 2.0 ** -53
LD = np.longdouble
SPREAD = NL.SPREAD

# (m, n): the smallest shapes at which each path of lse_hv_onepass_kernel<KCH> can go wrong
SHAPES_KCH1 = [(1, 1), (3, 5), (96, 64), (40, 65), (257, 200)]  # (3, 5), (1, 1): fewer rows than workgroups -- workgroups that own no row
SHAPES_WIDE = [(7, 1030), (5, 2050), (5, 4099), (3, 8200), (3, 16384)]  # KCH = 2, 4, 8, 16, 16 (the last: n_pad at its limit)
SHAPES_TALL = [(1024, 1024)]  # 256 workgroups of four rows each
SHAPES = SHAPES_KCH1 + SHAPES_WIDE + SHAPES_TALL
MASK_SHAPE = (96, 64)
MASK_ROWS = {"first": 0, "middle": 47, "last": 95}
SCALES = [1.0, SPREAD]
TOO_WIDE = 16400  # n_pad > 16384: the product is not built


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


@functools.lru_cache(maxsize=None)
def problem(m, n, masked=None):
    """(a, c, mu, x0, v) of spg_cases.lse_problem(m, n), with c[masked] = -inf if asked for; read-only, computed once."""
    a, c, mu, x0 = NL.problem(m, n)
    if masked is not None:
        c = c.copy()
        c[masked] = -np.inf
        c.setflags(write=False)
    v = np.random.default_rng(1000 * m + n).standard_normal(n)
    v.setflags(write=False)
    return a, c, mu, x0, v


def weights(a, c, x):
    """p = softmax(A x + c) and gbar = A'p in longdouble"""
    al, cl, xl = a.astype(LD), c.astype(LD), x.astype(LD)
    z = al @ xl + cl
    e = np.exp(z - z.max())
    p = e / e.sum()
    return al, p, al.T @ p


def truth_and_bound(a, c, mu, x, v):
    """(q*, c*, bound on q per entry, bound on c, (S |v|)) -- q* and c* in longdouble, the bounds in longdouble, the reference's share included"""
    m, n = a.shape
    al, p, gbar = weights(a, c, x)
    vl = v.astype(LD)
    u = al @ vl
    w = p * u
    q = al.T @ w - gbar * w.sum() + LD(mu) * vl
    cstar = vl @ q
    aa, av = np.abs(a), np.abs(v)
    p64 = p.astype(np.float64)
    uk = aa @ av
    g_abs = aa.T @ p64
    sv = aa.T @ (p64 * uk) + g_abs * float(g_abs @ av) + mu * av
    live = np.isfinite(c)
    zcap = float(np.max(aa[live] @ np.abs(x) + np.abs(c[live])))
    b = (2 * m + 4 * (n + 1) * zcap + 16) * U  # newton_lse_cases.hessian_truth_and_bound's B
    bv = 2.0 * b + (n + 4) * U
    ref = 1.0 + 2.0 ** -11  # the longdouble evaluation's own error: the same expressions with 2^-64 for u
    e_q = LD(bv * ref) * sv.astype(LD)
    vq = float(np.sum(av * np.abs(q.astype(np.float64))))
    c_bound = float(np.sum(av * e_q.astype(np.float64))) + gamma(n + 2) * ref * vq
    return q, cstar, e_q, LD(c_bound), sv


_truths = {}


def truth_at(m, n, scale, masked=None):
    """truth_and_bound of problem(m, n, masked) at scale * x0, computed once: (x, v) + its five results"""
    key = (m, n, scale, masked)
    if key not in _truths:
        a, c, mu, x0, v = problem(m, n, masked)
        x = scale * x0
        _truths[key] = (x, v) + truth_and_bound(a, c, mu, x, v)
    return _truths[key]


def hv_f64(a, c, mu, x, v, dot=np.dot, drop_gbar=False, normalise=True):
    """the product in float64 with the inner products made by `dot` (a summation order): what a correct float64 implementation computes;
    drop_gbar / normalise=False plant the faults the bound has to reject"""
    m, n = a.shape
    z = np.array([dot(a[k], x) for k in range(m)]) + c
    e = np.exp(z - z.max())
    p = e / dot(e, np.ones(m)) if normalise else e
    u = np.array([dot(a[k], v) for k in range(m)])
    w = p * u
    at = np.ascontiguousarray(a.T)
    gbar = np.array([dot(at[j], p) for j in range(n)])
    first = np.array([dot(at[j], w) for j in range(n)])
    ubar = dot(w, np.ones(m))
    q = first + mu * v if drop_gbar else (first - ubar * gbar) + mu * v
    return q, dot(v, q)
