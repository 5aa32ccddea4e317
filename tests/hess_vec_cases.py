"""The problems and the derived bounds the Hessian-vector tests share (tests/test_ref_hess_vec.py checks the derivations on the host in three
summation orders, tests/test_gpu_hess_vec.py holds qn_objective_hess_vec to them): q = Q v and c = v'Qv for a sparse Q in CSR and for a dense Q.
numpy only; the sparse matrices are tests/sparse_cases.py's.

THE BOUNDS are derived, not measured, and hold for any summation order, with or without FMA.  u = 2^-53, L_i the length of row i,
gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and 3.4):

    q_i   a sum of L_i products: |q_i - q_i*| <= gamma_(L_i) sum_j |Q_ij v_j|, stated with gamma_(L_i + 1) as tests/test_gpu_sparse.py states it for
          g_i = q_i - b_i with b = 0.  E(q_i) is this bound.
    c     the computed c is a sum of n products v_i q_i of the COMPUTED q_i: |c - sum_i v_i q_i| <= gamma_n sum_i |v_i q_i| (n - 1 additions at the
          most in front of any term in any tree, one rounding for the product), and |sum_i v_i (q_i - q_i*)| <= sum_i |v_i| E(q_i).  Stated as
          sum_i |v_i| E(q_i) + gamma_(n + 2) sum_i |v_i q_i*|: the two spare u cover |q_i| <= |q_i*| + E(q_i) in the first term, a product of two
          gammas.

The reference is np.longdouble (u = 2^-64; mpmath with 200 bits at n <= 7): its own error -- the same expressions with 2^-64 for u -- and the rounding
of the starred values to float64 (u per value) are added to the bounds."""
import functools

import numpy as np

import sparse_cases as SC

U = 2.0 ** -53
U_LD = 2.0 ** -64
LANES = (0, 1, 2, 4, 8, 16, 32, 64)


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


def small_7():
    """n = 7: row 0 full, row 3 empty, the others a diagonal and one more entry; not symmetric (multiplied as given).  tests/test_gpu_sparse.py's."""
    rows = [0] * 7 + [1, 1, 2, 2, 4, 4, 5, 5, 6, 6]
    cols = list(range(7)) + [1, 4, 0, 2, 4, 6, 3, 5, 2, 6]
    vals = [1.5, -0.25, 0.125, 3.0, -2.0, 0.75, 1e-3] + [2.0, -1.0, 0.5, 4.0, 1.25, -3.0, 0.3, 2.5, -0.7, 5.0]
    return SC.from_triplets(7, rows, cols, vals)


SPARSE_CASES = {
    "n1": lambda: (np.array([0, 1]), np.array([0]), np.array([2.5])),
    "n7_empty_and_full_row": small_7,
    "tri2050": lambda: SC.tri(2050),
    "arrow4100": lambda: SC.arrow(4100),  # (row 0 is longer than the long-row threshold of 2048)
    "band2050_350": lambda: SC.band(2050, 350),
    "nnz0": lambda: (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)),
    "tri_2p21_plus_2": lambda: SC.tri(SC.BIG_N),
}
HOST_CASES = [k for k in SPARSE_CASES if k != "tri_2p21_plus_2"]  # what the host check of the derivations runs
DENSE_SIZES = (2, 7, 2050)


def dense_matrix(n):
    """a dense symmetric matrix with entries of both signs, diagonally dominant"""
    a = np.random.default_rng(23).standard_normal((n, n))
    q = 0.5 * (a + a.T)
    q[np.arange(n), np.arange(n)] = np.abs(q).sum(axis=1) + 0.04
    return q


def dense_as_csr(q):
    n = q.shape[0]
    return np.arange(0, n * n + 1, n, dtype=np.int64), np.tile(np.arange(n, dtype=np.int64), n), q.reshape(-1).copy()


def vector(n):
    return np.random.default_rng(17).standard_normal(n)


def reference(csr, v):
    """(q*, c*, bound on q per row, bound on c): the starred values in float64 nearest to the extended-precision ones"""
    indptr, cols, vals = (np.asarray(a) for a in csr)
    indptr, cols = indptr.astype(np.int64), cols.astype(np.int64)
    n = indptr.size - 1
    lens = np.diff(indptr)
    rows = SC.row_index(indptr)
    absq = np.bincount(rows, weights=np.abs(vals * v[cols]), minlength=n)
    if n <= 7:
        import mpmath
        mpmath.mp.prec = 200
        q = [mpmath.mpf(0)] * n
        for r, c, a in zip(rows, cols, vals):
            q[r] += mpmath.mpf(float(a)) * mpmath.mpf(float(v[c]))
        q_ref = np.array([float(qi) for qi in q])
        c_ref = float(sum((mpmath.mpf(float(v[i])) * q[i] for i in range(n)), mpmath.mpf(0)))
        u_ref = 0.0
    else:
        prod = vals.astype(np.longdouble) * v[cols].astype(np.longdouble)
        q = np.zeros(n, dtype=np.longdouble)
        nonempty = lens > 0
        q[nonempty] = np.add.reduceat(prod, indptr[:-1][nonempty])  # (consecutive non-empty rows' starts delimit each row's entries)
        q_ref = q.astype(np.float64)
        c_ref = float(np.sum(v.astype(np.longdouble) * q))
        u_ref = U_LD
    e_q = np.array([gamma(int(k) + 1) for k in lens]) * absq  # E(q_i): the code under test's share
    e_q_ref = np.array([gamma(int(k) + 1, u_ref) for k in lens]) * absq if u_ref else np.zeros(n)
    q_bound = e_q + e_q_ref + U * np.abs(q_ref)
    vq = float(np.sum(np.abs(v) * np.abs(q_ref)))
    c_bound = float(np.sum(np.abs(v) * e_q)) + gamma(n + 2) * vq
    if u_ref:
        c_bound += float(np.sum(np.abs(v) * e_q_ref)) + gamma(n + 2, u_ref) * vq
    c_bound += U * abs(c_ref)
    return q_ref, c_ref, q_bound, c_bound


@functools.lru_cache(maxsize=None)
def sparse_reference(name):
    """(csr with int64 indices, v, q*, c*, bound on q, bound on c) of one sparse case: computed once, shared, never written to"""
    indptr, cols, vals = (np.asarray(a) for a in SPARSE_CASES[name]())
    csr = (indptr.astype(np.int64), cols.astype(np.int64), vals.astype(np.float64))
    v = vector(csr[0].size - 1)
    return (csr, v) + reference(csr, v)


@functools.lru_cache(maxsize=None)
def dense_reference(n):
    q = dense_matrix(n)
    v = vector(n)
    return (q, v) + reference(dense_as_csr(q), v)
