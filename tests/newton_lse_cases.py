"""What tests/test_ref_newton_lse.py (CPU) and tests/test_gpu_newton_lse.py (GPU) share: Newton on the log-sum-exp problems of
spg_cases.lse_problem, the oracle's run of each case, and the extended-precision Hessian with its derived error bound."""
import functools

import numpy as np

import pnewton_cases as PC
import spg_cases as S

TOL = 1e-10
MAX_ITER, MAX_LS = 50, 20
HESS_SHAPES = [(1, 1), (3, 5), (96, 64), (40, 65), (257, 200), (1024, 1024)]  # (m, n)
RUN_SHAPES = [(96, 64), (257, 200)]
LU_SHAPE = (96, 64)
# At x0 (standard normal entries) z = A x0 has a spread of about sqrt(n): from n = 200 on the softmax sits on a few rows and the others' masks
# cannot be seen in H.  The Hessian is therefore also looked at SPREAD * x0, where every row carries a weight of about 1 / m.
SPREAD = 0.01
ITER_BOUND = 15  # "well inside the cap" of 50: a plain numpy Newton takes 8-9 iterations on these problems


@functools.lru_cache(maxsize=None)
def problem(m, n):
    a, c, mu, x0, _, _ = S.lse_problem(m, n)
    for v in (a, c, x0):
        v.setflags(write=False)
    return a, c, mu, x0


def ls_of(mod, name):
    if name == "mt":
        return mod.MoreThuente() if hasattr(mod, "MoreThuente") else mod.morethuente()
    return mod.BackTracking(1e-4, 0.5) if hasattr(mod, "BackTracking") else mod.backtracking(1e-4, 0.5)


_oracle_runs = {}


def oracle_run(qo, m, n, lsname):
    """The CPU oracle's Newton on the case: (status, k, t of the first iteration, x).  Computed once per case."""
    key = (m, n, lsname)
    if key not in _oracle_runs:
        a, c, mu, x0 = problem(m, n)
        fn = PC.lse_hess_fn(a, c, mu)
        ref = qo.Solver(qo.NEWTON, TOL, x0)
        ref.set_hessian(lambda x: fn(x)[2])
        st = ref.minimize(ls_of(qo, lsname), qo.LogSumExpOracle(a, c, mu), MAX_ITER, MAX_LS, trace_cap=MAX_ITER, trace_x=False)
        x = ref.x
        x.setflags(write=False)
        _oracle_runs[key] = (st, ref.k, ref.trace[0]["t"] if ref.trace else None, x)
    return _oracle_runs[key]


def hessian_truth_and_bound(a, c, mu, x):
    """H = A'(diag(p) - p p')A + mu I in np.longdouble from the same a, c, x (the lower block triangle is evaluated, the upper one is its
    mirror image: the formula is symmetric term by term), and the entrywise bound B * S_ij of DESIGN.md 20:
    S_ij = sum_k p_k |a_ki| |a_kj| + G_i G_j + mu delta_ij, G = |A|'p, B = (2m + 4(n + 1) Z + 16) 2^-53, Z = max_k (sum_j |a_kj x_j| + |c_k|).
    (S is the scale of a bound, not a reference: it is summed in f64 from the longdouble weights.)"""
    L = np.longdouble
    al, cl, xl = a.astype(L), c.astype(L), x.astype(L)
    m, n = a.shape
    z = al @ xl + cl
    e = np.exp(z - z.max())
    p = e / e.sum()
    gbar = al.T @ p
    pa = (al.T * p)
    h = np.empty((n, n), dtype=L)
    blk = 128
    for i0 in range(0, n, blk):
        for j0 in range(0, i0 + 1, blk):
            t = pa[i0:i0 + blk] @ al[:, j0:j0 + blk]
            h[i0:i0 + blk, j0:j0 + blk] = t
            if j0 != i0:
                h[j0:j0 + blk, i0:i0 + blk] = t.T
    il = np.tril_indices(n, -1)
    h[il[1], il[0]] = h[il]  # (inside the diagonal blocks too: one value per unordered pair)
    h = h - np.outer(gbar, gbar) + L(mu) * np.eye(n, dtype=L)
    aa = np.abs(a)
    p64 = p.astype(np.float64)
    g_abs = aa.T @ p64
    s = (aa.T * p64) @ aa + np.outer(g_abs, g_abs) + mu * np.eye(n)
    zcap = float(np.max(np.abs(al) @ np.abs(xl) + np.abs(cl)))
    b = (2 * m + 4 * (n + 1) * zcap + 16) * 2.0 ** -53
    return h, L(b) * s.astype(L), s.astype(L)


_truths = {}


def truth_at(m, n, scale):
    """hessian_truth_and_bound of problem(m, n) at scale * x0, computed once."""
    if (m, n, scale) not in _truths:
        a, c, mu, x0 = problem(m, n)
        _truths[(m, n, scale)] = hessian_truth_and_bound(a, c, mu, scale * x0)
    return _truths[(m, n, scale)]


def x_floor(n, x):
    return n * 2.0 ** -52 * max(1.0, float(np.linalg.norm(x)))
