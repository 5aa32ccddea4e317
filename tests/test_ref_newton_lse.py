"""CPU companion of tests/test_gpu_newton_lse.py: the oracle (qo) alone licenses the cases the GPU file runs -- Newton with the analytic
log-sum-exp Hessian (pnewton_cases.lse_hess_fn) on qo.LogSumExpOracle returns OK well inside the iteration cap on every case --, and the
extended-precision Hessian and its bound (newton_lse_cases.hessian_truth_and_bound) are checked against numpy's own f64 evaluation."""
import numpy as np
import pytest

import newton_lse_cases as NC
import pnewton_cases as PC


@pytest.mark.parametrize("lsname", ["mt", "bt"])
@pytest.mark.parametrize("m,n", NC.RUN_SHAPES + [(40, 65)])
def test_oracle_newton_converges_well_inside_the_cap(qo, m, n, lsname):
    a, c, mu, x0 = NC.problem(m, n)
    st, k, t0, x = NC.oracle_run(qo, m, n, lsname)
    print(f"oracle Newton ({m}, {n}) {lsname}: status={st} k={k} t0={t0}")
    assert st == qo.OK and 1 <= k <= NC.ITER_BOUND
    f, g, h = PC.lse_hess_fn(a, c, mu)(x)
    assert 0.5 * float(g @ np.linalg.solve(h, g)) < NC.TOL  # Newton's own test (newton/mod.rs:65-66: half the squared decrement) holds at the end point
    assert np.linalg.cond(h) < 100.0  # (about 10 on these problems: the factorisation adds little to the distances the GPU file compares)


@pytest.mark.parametrize("m,n", NC.HESS_SHAPES[:-1])  # (the largest shape's extended-precision products take seconds: the GPU file computes them once)
def test_f64_hessian_sits_inside_the_derived_bound(m, n):
    """numpy's f64 evaluation against the longdouble truth, in units of 2^-53 S_ij: a few units, far inside B (which grows with m and n Z)."""
    a, c, mu, x0 = NC.problem(m, n)
    truth, bound, s = NC.hessian_truth_and_bound(a, c, mu, x0)
    h64 = PC.lse_hess_fn(a, c, mu)(x0)[2]
    err = np.abs(h64.astype(np.longdouble) - truth)
    units = float(np.max(err / (s * 2.0 ** -53)))
    print(f"({m}, {n}): f64 numpy max error {units:.2f} units of 2^-53 S_ij; bound {float(np.max(bound / s)) * 2.0 ** 53:.0f} units")
    assert np.all(err <= bound)
    assert units <= 64.0
    # what the bound is for: a dropped row that carries weight (at SPREAD * x0 every row does: about 1 / m each) lands orders of magnitude outside it
    if m >= 3:
        xs = NC.SPREAD * x0
        truth_s, bound_s, _ = NC.hessian_truth_and_bound(a, c, mu, xs)
        dropped = PC.lse_hess_fn(a[:-1], c[:-1], mu)(xs)[2]
        assert np.any(np.abs(dropped.astype(np.longdouble) - truth_s) > 1e3 * bound_s)


def test_saturated_softmax_truth_is_mu_identity():
    a, c, mu, x0 = NC.problem(96, 64)
    c = c.copy()
    c[17] += 800.0
    truth, bound, _ = NC.hessian_truth_and_bound(a, c, mu, x0)
    assert np.all(np.isfinite(truth.astype(np.float64)))
    assert np.max(np.abs(truth - mu * np.eye(64))) <= 1e-300
