"""CPU companion of tests/test_gpu_lse_hess_vec.py: the derived bound of tests/lse_hess_vec_cases.py is checked on the host, with no
GPU and nothing from the code under test.  A correct float64 evaluation of H(x) v = A'(p o (A v)) - gbar (p . (A v)) + mu v sits inside it in three
summation orders (numpy.dot, math.fsum, reversed); planted faults -- the `- ubar gbar` term dropped, a row dropped, p not normalised -- land far
outside it where every row carries weight (at SPREAD * x0); the matrix-free truth agrees with the dense Hessian's truth of newton_lse_cases.py."""
import math

import numpy as np
import pytest

import lse_hess_vec_cases as HV
import newton_lse_cases as NL

ORDERS = {
    "numpy": np.dot,
    "fsum": lambda a, b: math.fsum(np.asarray(a) * np.asarray(b)),
    "reversed": lambda a, b: float(np.dot(np.asarray(a)[::-1], np.asarray(b)[::-1])),
}
HOST_SHAPES = HV.SHAPES_KCH1 + [(7, 1030), (5, 2050)]  # (the wider shapes add nothing on the host: the bound's n and Z are the same expressions)


@pytest.mark.parametrize("scale", HV.SCALES, ids=["x0", "spread"])
@pytest.mark.parametrize("m,n", HOST_SHAPES)
def test_f64_product_sits_inside_the_derived_bound_in_three_orders(m, n, scale):
    a, c, mu, x0, _ = HV.problem(m, n)
    x, v, q_ref, c_ref, q_bound, c_bound, sv = HV.truth_at(m, n, scale)
    for name, dot in ORDERS.items():
        q, cc = HV.hv_f64(a, c, mu, x, v, dot=dot)
        err = np.abs(q.astype(HV.LD) - q_ref)
        units = float(np.max(err / (sv.astype(HV.LD) * HV.U)))
        print(f"({m}, {n}) scale={scale} {name}: max error {units:.2f} units of 2^-53 (S|v|)_j, bound {float(np.max(q_bound / sv)) / HV.U:.0f}; "
              f"|c - c*| / bound = {float(abs(HV.LD(cc) - c_ref) / c_bound):.2e}")
        assert np.all(err <= q_bound), name
        assert abs(HV.LD(cc) - c_ref) <= c_bound, name
        assert units <= 256.0, name  # a correct evaluation is a few units; the bound grows with m and n Z


@pytest.mark.parametrize("m,n", [(3, 5), (96, 64), (40, 65), (257, 200)])
def test_planted_faults_are_rejected(m, n):
    a, c, mu, x0, _ = HV.problem(m, n)
    x, v, q_ref, c_ref, q_bound, c_bound, _ = HV.truth_at(m, n, HV.SPREAD)

    def outside(q):
        return float(np.max(np.abs(q.astype(HV.LD) - q_ref) / q_bound))
    good, _ = HV.hv_f64(a, c, mu, x, v)
    assert outside(good) <= 1.0
    no_gbar, c_no_gbar = HV.hv_f64(a, c, mu, x, v, drop_gbar=True)
    assert outside(no_gbar) > 1e3
    assert abs(HV.LD(c_no_gbar) - c_ref) > 1e3 * c_bound
    dropped, _ = HV.hv_f64(a[:-1], c[:-1], mu, x, v)
    assert outside(dropped) > 1e3
    unnormalised, _ = HV.hv_f64(a, c, mu, x, v, normalise=False)
    assert outside(unnormalised) > 1e3


@pytest.mark.parametrize("m,n", [(3, 5), (96, 64), (40, 65)])
def test_matrix_free_truth_is_the_dense_truth_times_v(m, n):
    """two longdouble evaluations of the same quantity -- H* v from newton_lse_cases' matrix, and the matrix-free form -- inside twice the
    reference's own share of the bound; and (S |v|) is that file's scale matrix times |v|"""
    for scale in HV.SCALES:
        x, v, q_ref, c_ref, q_bound, _, sv = HV.truth_at(m, n, scale)
        h, _, s = NL.truth_at(m, n, scale)
        hv = h @ v.astype(HV.LD)
        assert np.all(np.abs(hv - q_ref) <= 2.0 ** -10 * q_bound)
        assert np.allclose((s @ np.abs(v).astype(HV.LD)).astype(np.float64), sv, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("where", list(HV.MASK_ROWS))
def test_a_masked_row_is_a_dropped_row(where):
    """c_k = -inf: p_k = 0 exactly, the truth is the truth of the problem without that row, and Z does not see the row (the bound stays finite)"""
    m, n = HV.MASK_SHAPE
    k = HV.MASK_ROWS[where]
    a, c, mu, x0, v = HV.problem(m, n, k)
    x, _, q_ref, c_ref, q_bound, c_bound, _ = HV.truth_at(m, n, HV.SPREAD, k)
    assert np.all(np.isfinite(q_bound.astype(np.float64))) and np.isfinite(float(c_bound))
    keep = np.arange(m) != k
    q2, c2, _, _, _ = HV.truth_and_bound(a[keep], c[keep], mu, x, v)
    assert np.all(np.abs(q2 - q_ref) <= 2.0 ** -10 * q_bound)
    full = HV.truth_at(m, n, HV.SPREAD)[2]
    assert np.any(np.abs(full - q_ref) > 1e3 * q_bound)  # (and the mask can be seen: the unmasked problem is another one)
