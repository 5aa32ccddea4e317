"""GPU tests of the curvature pass of the device quadratics, q = Q v and c = v'Qv (qn_objective_hess_vec, Objective.hess_vec; kernels
csrc/qn_sparse.hip.h spq_curv_kernel and csrc/qn_vec_exact.hip.h): against extended precision with the derived bounds of tests/hess_vec_cases.py
(checked on the host by tests/test_ref_hess_vec.py; no tolerance comes from the code under test), bit for bit against the evaluation kernel
(q is what an evaluation at v with b = 0 returns as g), its determinism, and its error paths."""
import numpy as np
import pytest

import hess_vec_cases as HC

pytestmark = pytest.mark.gpu


def _worst(err, bound):
    return float(np.max(err / np.where(bound > 0.0, bound, 1.0))) if err.size else 0.0


# ---- 1. against extended precision ----
@pytest.mark.parametrize("index_type", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("name", list(HC.SPARSE_CASES))
def test_sparse_hess_vec_against_extended_precision(qn, name, index_type):
    (indptr, cols, vals), v, q_ref, c_ref, q_bound, c_bound = HC.sparse_reference(name)
    obj = qn.SparseQuadratic(indptr.astype(index_type), cols.astype(index_type), vals, np.zeros(v.size))
    try:
        if name == "arrow4100":
            assert obj.n_long_rows >= 1
        worst_q = worst_c = 0.0
        for lanes in HC.LANES:
            obj.set_lanes_per_row(lanes)
            q, c = obj.hess_vec(v)
            err = np.abs(q - q_ref)
            worst_q = max(worst_q, _worst(err, q_bound))
            worst_c = max(worst_c, abs(c - c_ref) / c_bound if c_bound > 0.0 else abs(c - c_ref))
            assert np.all(err <= q_bound), (lanes, int(np.argmax(err - q_bound)), float(np.max(err - q_bound)))
            assert abs(c - c_ref) <= c_bound, (lanes, c, c_ref, c_bound)
            if name == "nnz0":
                assert not q.any() and c == 0.0
            # the same launches without the download of q: the same c
            none, c2 = obj.hess_vec(v, download=False)
            assert none is None and np.float64(c2).tobytes() == np.float64(c).tobytes()
        print(f"hess_vec {name} {np.dtype(index_type).name}: worst |q - q*| / bound={worst_q:.3f} worst |c - c*| / bound={worst_c:.3f}")
    finally:
        obj.close()


@pytest.mark.parametrize("n", HC.DENSE_SIZES)
def test_dense_hess_vec_against_extended_precision(qn, n):
    qm, v, q_ref, c_ref, q_bound, c_bound = HC.dense_reference(n)
    obj = qn.Quadratic(qm, np.zeros(n))
    try:
        q, c = obj.hess_vec(v)
        err = np.abs(q - q_ref)
        print(f"hess_vec dense n={n}: worst |q - q*| / bound={_worst(err, q_bound):.3f} |c - c*| / bound={abs(c - c_ref) / c_bound:.3f}")
        assert np.all(err <= q_bound), (int(np.argmax(err - q_bound)), float(np.max(err - q_bound)))
        assert abs(c - c_ref) <= c_bound, (c, c_ref, c_bound)
    finally:
        obj.close()


# ---- 2. the curvature pass keeps the evaluation's summation order: q is g of an evaluation at v with b = 0, bit for bit ----
@pytest.mark.parametrize("name", ["n7_empty_and_full_row", "tri2050", "arrow4100", "band2050_350"])
def test_sparse_q_has_the_bits_of_the_evaluation(qn, name):
    (indptr, cols, vals), v, _, _, _, _ = HC.sparse_reference(name)
    obj = qn.SparseQuadratic(indptr, cols, vals, np.zeros(v.size))
    try:
        for lanes in HC.LANES:
            obj.set_lanes_per_row(lanes)
            q, _ = obj.hess_vec(v)
            _, g = obj(v)
            assert q.tobytes() == g.tobytes(), lanes  # (g_i = q_i - 0 is q_i, and an empty row's +0 - 0 is the +0 the curvature pass stores)
    finally:
        obj.close()


@pytest.mark.parametrize("n", HC.DENSE_SIZES)
def test_dense_q_has_the_bits_of_the_evaluation(qn, n):
    qm, v, _, _, _, _ = HC.dense_reference(n)
    obj = qn.Quadratic(qm, np.zeros(n))
    try:
        q, _ = obj.hess_vec(v)
        _, g = obj(v)
        assert q.tobytes() == g.tobytes()
    finally:
        obj.close()


def test_hess_vec_leaves_the_evaluation_alone(qn):
    """the two share scratch buffers on one stream: f and g before and after a curvature pass are the same bits, with b in play"""
    (indptr, cols, vals), v, _, _, _, _ = HC.sparse_reference("arrow4100")
    b = np.random.default_rng(5).standard_normal(v.size)
    obj = qn.SparseQuadratic(indptr, cols, vals, b)
    try:
        f1, g1 = obj(v)
        q, c = obj.hess_vec(2.0 * v)
        f2, g2 = obj(v)
        assert np.float64(f1).tobytes() == np.float64(f2).tobytes() and g1.tobytes() == g2.tobytes()
        q1, c1 = obj.hess_vec(v)
        assert (2.0 * q1).tobytes() == q.tobytes()  # (a factor of two is exact in every product and sum)
        assert 4.0 * c1 == c
    finally:
        obj.close()


# ---- 3. determinism: two calls, and two objects from the same arrays ----
@pytest.mark.parametrize("name", ["arrow4100", "band2050_350", "tri_2p21_plus_2"])
def test_sparse_determinism(qn, name):
    (indptr, cols, vals), v, _, _, _, _ = HC.sparse_reference(name)
    b = np.zeros(v.size)
    one, two = qn.SparseQuadratic(indptr, cols, vals, b), qn.SparseQuadratic(indptr.copy(), cols.copy(), vals.copy(), b.copy())
    try:
        for lanes in (0, 2, 64):
            one.set_lanes_per_row(lanes)
            two.set_lanes_per_row(lanes)
            (q1, c1), (q2, c2), (q3, c3) = one.hess_vec(v), one.hess_vec(v), two.hess_vec(v)
            assert np.float64(c1).tobytes() == np.float64(c2).tobytes() == np.float64(c3).tobytes()
            assert q1.tobytes() == q2.tobytes() == q3.tobytes()
    finally:
        one.close()
        two.close()


def test_dense_determinism(qn):
    qm, v, _, _, _, _ = HC.dense_reference(2050)
    one, two = qn.Quadratic(qm, np.zeros(2050)), qn.Quadratic(qm.copy(), np.zeros(2050))
    try:
        (q1, c1), (q2, c2), (q3, c3) = one.hess_vec(v), one.hess_vec(v), two.hess_vec(v)
        assert np.float64(c1).tobytes() == np.float64(c2).tobytes() == np.float64(c3).tobytes()
        assert q1.tobytes() == q2.tobytes() == q3.tobytes()
    finally:
        one.close()
        two.close()


# ---- 4. error paths ----
def test_error_paths(qn):
    rng = np.random.default_rng(3)
    lse = qn.LogSumExp(rng.standard_normal((5, 4)), rng.standard_normal(5), 0.1)
    try:
        with pytest.raises(qn.ErrorInputParams, match="not built"):
            lse.hess_vec(np.ones(4))
    finally:
        lse.close()
    obj = qn.Quadratic(np.eye(3), np.zeros(3))
    try:
        with pytest.raises(qn.ErrorInputParams, match="entries"):
            obj.hess_vec(np.ones(4))
        q, c = obj.hess_vec(np.array([1.0, -2.0, 3.0]))
        assert np.array_equal(q, [1.0, -2.0, 3.0]) and c == 14.0
    finally:
        obj.close()
    with pytest.raises(qn.ErrorInputParams, match="closed"):
        obj.hess_vec(np.ones(3))
