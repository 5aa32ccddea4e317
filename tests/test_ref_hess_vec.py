"""CPU check of the two derived bounds of tests/hess_vec_cases.py (on q = Q v per row, on c = v'Qv): float64 results formed on the host in three
summation orders -- storage order with numpy.dot, every sum reversed, and math.fsum (every sum exact, rounded once) -- must all fall inside the bounds
around the extended-precision reference, and the bounds must be tight enough to mean something.  No GPU, no library."""
import math

import numpy as np
import pytest

import hess_vec_cases as HC
import sparse_cases as SC


def _orders(csr, v):
    """[(name, q, c)] in float64"""
    indptr, cols, vals = csr
    n = indptr.size - 1
    out = []
    q = SC.matvec(csr, v) if vals.size else np.zeros(n)
    out.append(("storage order, numpy.dot", q, float(np.dot(v, q))))
    qr = SC.matvec(csr, v, reverse=True) if vals.size else np.zeros(n)
    out.append(("reversed", qr, SC.rev_dot(v, qr)))
    prod = vals * v[cols]
    qf = np.array([math.fsum(prod[indptr[i]:indptr[i + 1]]) for i in range(n)])
    out.append(("math.fsum", qf, math.fsum(v * qf)))
    return out


def _check(csr, v, q_ref, c_ref, q_bound, c_bound, label):
    for name, q, c in _orders(csr, v):
        err = np.abs(q - q_ref)
        assert np.all(err <= q_bound), (label, name, int(np.argmax(err - q_bound)))
        assert abs(c - c_ref) <= c_bound, (label, name, c, c_ref, c_bound)
    # a bound that admits a wrong answer shows nothing: one entry of Q off by one part in 10^6 of its row's scale must break it
    scale = np.abs(q_ref).max() if q_ref.size else 0.0
    if scale > 0.0:
        assert np.all(q_bound <= 1e-9 * max(scale, 1.0)), label
        assert c_bound <= 1e-9 * max(abs(c_ref), float(np.sum(np.abs(v) * np.abs(q_ref)))), label


@pytest.mark.parametrize("name", HC.HOST_CASES)
def test_bounds_hold_in_three_summation_orders_sparse(name):
    csr, v, q_ref, c_ref, q_bound, c_bound = HC.sparse_reference(name)
    _check(csr, v, q_ref, c_ref, q_bound, c_bound, name)
    if name == "nnz0":
        assert not q_ref.any() and c_ref == 0.0 and not q_bound.any() and c_bound == 0.0


@pytest.mark.parametrize("n", HC.DENSE_SIZES)
def test_bounds_hold_in_three_summation_orders_dense(n):
    q, v, q_ref, c_ref, q_bound, c_bound = HC.dense_reference(n)
    _check(HC.dense_as_csr(q), v, q_ref, c_ref, q_bound, c_bound, f"dense{n}")
    # the dense product as numpy forms it (BLAS: blocked, fused multiply-adds) is a fourth order
    qd = q @ v
    assert np.all(np.abs(qd - q_ref) <= q_bound)
    assert abs(float(v @ qd) - c_ref) <= c_bound


def test_curvature_of_a_positive_definite_matrix_is_positive():
    """the references themselves: tri and band are SPD, so c* > 0; and c* is v'q* to the bound"""
    for name in ("tri2050", "band2050_350", "arrow4100"):
        _, v, q_ref, c_ref, _, c_bound = HC.sparse_reference(name)
        assert c_ref > 0.0
        assert abs(math.fsum(v * q_ref) - c_ref) <= c_bound
