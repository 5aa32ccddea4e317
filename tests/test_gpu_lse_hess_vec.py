"""GPU tests of the log-sum-exp Hessian-vector product q = H(x) v, c = v'H(x)v (qn_objective_hess_vec_at, Objective.hess_vec_at; kernels
csrc/qn_lse_hv.hip.h): against np.longdouble with the derived element-wise bound of tests/lse_hess_vec_cases.py (checked on the host
by tests/test_ref_lse_hess_vec.py -- no tolerance comes from the code under test) on the smallest shapes at which each instance of the kernel can
go wrong, against the dense Hessian's columns, its symmetry, its determinism, what it leaves of the evaluation, and its error paths."""
import numpy as np
import pytest

import hess_vec_cases as HC
import lse_hess_vec_cases as HV
import newton_lse_cases as NL

pytestmark = pytest.mark.gpu
LD = HV.LD


def _check(q, c, truth, label):
    _, _, q_ref, c_ref, q_bound, c_bound, sv = truth
    err = np.abs(q.astype(LD) - q_ref)
    units = float(np.max(err / (sv.astype(LD) * HV.U)))
    c_err = abs(LD(c) - c_ref)
    print(f"hess_vec_at {label}: max |q - q*| = {units:.2f} units of 2^-53 (S|v|)_j (bound {float(np.max(q_bound / sv)) / HV.U:.0f}); "
          f"|c - c*| / bound = {float(c_err / c_bound):.2e}")
    assert np.all(np.isfinite(q)) and np.isfinite(c)
    assert np.all(err <= q_bound), (label, int(np.argmax(err - q_bound)), float(np.max(err / q_bound)))
    assert c_err <= c_bound, (label, c, float(c_ref), float(c_bound))


# ---- 1. against extended precision: every instance (KCH = 1, 2, 4, 8, 16), workgroups without rows, several rows per workgroup ----
@pytest.mark.parametrize("m,n", HV.SHAPES)
def test_against_extended_precision(qn, m, n):
    a, c, mu, x0, v = HV.problem(m, n)
    obj = qn.LogSumExp(a, c, mu)
    try:
        for scale in HV.SCALES:
            truth = HV.truth_at(m, n, scale)
            q, vhv = obj.hess_vec_at(truth[0], v)
            _check(q, vhv, truth, f"({m}, {n}) at {scale} x0")
            none, vhv2 = obj.hess_vec_at(truth[0], v, download=False)  # the same launches without the download of q: the same c
            assert none is None and np.float64(vhv2).tobytes() == np.float64(vhv).tobytes()
    finally:
        obj.close()


@pytest.mark.parametrize("where", list(HV.MASK_ROWS))
def test_a_masked_row_adds_nothing(qn, where):
    m, n = HV.MASK_SHAPE
    k = HV.MASK_ROWS[where]
    a, c, mu, x0, v = HV.problem(m, n, k)
    obj = qn.LogSumExp(a, c, mu)
    try:
        for scale in HV.SCALES:
            truth = HV.truth_at(m, n, scale, k)
            q, vhv = obj.hess_vec_at(truth[0], v)
            _check(q, vhv, truth, f"({m}, {n}) row {k} masked, at {scale} x0")
    finally:
        obj.close()


# ---- 2. against the dense Hessian the device forms, column by column, and its symmetry ----
@pytest.mark.parametrize("m,n", [(3, 5), (40, 65)])
def test_unit_vectors_give_the_columns_of_the_hessian(qn, m, n):
    a, c, mu, x0, _ = HV.problem(m, n)
    obj = qn.LogSumExp(a, c, mu)
    try:
        for scale in HV.SCALES:
            x = scale * x0
            h = obj.hessian(x)
            _, h_bound, s = NL.truth_at(m, n, scale)
            for j in range(n):
                e = np.zeros(n)
                e[j] = 1.0
                q, vhv = obj.hess_vec_at(x, e)
                bound = h_bound[:, j] + HV.truth_and_bound(a, c, mu, x, e)[2]  # the sum of both bounds
                assert np.all(np.abs(q.astype(LD) - h[:, j].astype(LD)) <= bound), (scale, j)
                assert abs(LD(vhv) - LD(q[j])) == 0  # e_j' q: one product by 1 and zeros
    finally:
        obj.close()


@pytest.mark.parametrize("m,n", [(96, 64), (5, 2050)])
def test_the_product_is_symmetric_inside_the_bounds(qn, m, n):
    a, c, mu, x0, v = HV.problem(m, n)
    u = np.random.default_rng(7).standard_normal(n)
    obj = qn.LogSumExp(a, c, mu)
    try:
        x = HV.SPREAD * x0
        hv, _ = obj.hess_vec_at(x, v)
        hu, _ = obj.hess_vec_at(x, u)
        e_v, e_u = HV.truth_and_bound(a, c, mu, x, v)[2], HV.truth_and_bound(a, c, mu, x, u)[2]
        ul, vl = u.astype(LD), v.astype(LD)
        lhs, rhs = ul @ hv.astype(LD), vl @ hu.astype(LD)
        assert abs(lhs - rhs) <= np.abs(ul) @ e_v + np.abs(vl) @ e_u
    finally:
        obj.close()


# ---- 3. determinism; the evaluation is left alone; a quadratic's product is hess_vec's ----
@pytest.mark.parametrize("m,n", [(257, 200), (5, 4099), (1024, 1024)])
def test_determinism_across_calls_and_objects(qn, m, n):
    a, c, mu, x0, v = HV.problem(m, n)
    one, two = qn.LogSumExp(a, c, mu), qn.LogSumExp(a.copy(), c.copy(), mu)
    try:
        (q1, c1), (q2, c2), (q3, c3) = one.hess_vec_at(x0, v), one.hess_vec_at(x0, v), two.hess_vec_at(x0, v)
        assert np.float64(c1).tobytes() == np.float64(c2).tobytes() == np.float64(c3).tobytes()
        assert q1.tobytes() == q2.tobytes() == q3.tobytes()
    finally:
        one.close()
        two.close()


def test_the_evaluation_is_left_alone(qn):
    a, c, mu, x0, v = HV.problem(257, 200)
    obj = qn.LogSumExp(a, c, mu)
    try:
        f1, g1 = obj(x0)
        obj.hess_vec_at(0.5 * x0, v)
        f2, g2 = obj(x0)
        assert np.float64(f1).tobytes() == np.float64(f2).tobytes() and g1.tobytes() == g2.tobytes()
    finally:
        obj.close()


def test_on_a_quadratic_it_is_hess_vec(qn):
    qm, v, _, _, _, _ = HC.dense_reference(7)
    obj = qn.Quadratic(qm, np.zeros(7))
    try:
        (q1, c1), (q2, c2) = obj.hess_vec(v), obj.hess_vec_at(np.ones(7), v)
        assert q1.tobytes() == q2.tobytes() and np.float64(c1).tobytes() == np.float64(c2).tobytes()
    finally:
        obj.close()
    (indptr, cols, vals), v, _, _, _, _ = HC.sparse_reference("tri2050")
    sp = qn.SparseQuadratic(indptr, cols, vals, np.zeros(v.size))
    try:
        (q1, c1), (q2, c2) = sp.hess_vec(v), sp.hess_vec_at(np.ones(v.size), v)
        assert q1.tobytes() == q2.tobytes() and np.float64(c1).tobytes() == np.float64(c2).tobytes()
    finally:
        sp.close()


# ---- 4. error paths ----
def test_error_paths(qn):
    rng = np.random.default_rng(3)
    lse = qn.LogSumExp(rng.standard_normal((5, 4)), rng.standard_normal(5), 0.1)
    try:
        with pytest.raises(qn.ErrorInputParams, match="entries"):
            lse.hess_vec_at(np.ones(4), np.ones(5))
        with pytest.raises(qn.ErrorInputParams, match="entries"):
            lse.hess_vec_at(np.ones(3), np.ones(4))
        with pytest.raises(qn.ErrorInputParams, match="not built"):  # (qn_objective_hess_vec has no point to form p at)
            lse.hess_vec(np.ones(4))
    finally:
        lse.close()
    with pytest.raises(qn.ErrorInputParams, match="closed"):
        lse.hess_vec_at(np.ones(4), np.ones(4))
    wide = qn.LogSumExp(rng.standard_normal((2, HV.TOO_WIDE)), np.zeros(2), 0.1)
    try:
        with pytest.raises(qn.ErrorInputParams, match="not built"):
            wide.hess_vec_at(np.zeros(HV.TOO_WIDE), np.ones(HV.TOO_WIDE))
    finally:
        wide.close()


def test_a_row_sharded_context_is_refused(qn):
    """world = 2 through the host exchange, this rank alone: the objective is created (rank 0's rows) and the product refuses it before any launch"""
    def gather(send, recv):
        recv[:send.size] = send
        recv[send.size:] = send
    ctx = qn.Context(0, 0, 2, host_allgather=gather)
    try:
        rng = np.random.default_rng(5)
        obj = qn.LogSumExp(rng.standard_normal((32, 6)), rng.standard_normal(32), 0.1, ctx=ctx)
        try:
            with pytest.raises(qn.ErrorInputParams, match="single-GPU"):
                obj.hess_vec_at(np.zeros(6), np.ones(6))
        finally:
            obj.close()
    finally:
        ctx.close()
