"""CPU tests of tests/ref_prox.py, the restatement the GPU solver QN_SPECTRAL_PROXIMAL_GRADIENT is checked against: with l1 = 0 it IS
ref_spg.SpectralProjectedGradient, bit for bit; on separable quadratics it ends at the closed-form minimiser with exact zeros; the windows
tests/test_gpu_prox.py compares are the ones over which three summation orders take the same decisions; and five planted faults are each
rejected by a comparison the tests make."""
import numpy as np
import pytest

import prox_cases as PC
import ref_prox as RP
import ref_spg as R
import spg_cases as S


@pytest.mark.parametrize("box", [0.05, None])
def test_l1_zero_is_spg_bit_for_bit(qo, box):
    n, iters = 64, 30
    q, b, x0, _ = S.problem(qo, n)
    fn = R.quadratic_fn(q, b)
    lb, ub = S.bounds(n, box if box is not None else float("inf"))
    o1 = R.CountingOracle(fn)
    spg = R.SpectralProjectedGradient(1e-10, x0, o1, lb, ub)
    with pytest.raises(R.MaxIterReached):
        spg.minimize(R.GLLQuadratic(1e-4, 10), o1, iters, 50)
    o2 = R.CountingOracle(fn)
    prox = RP.SpectralProximalGradient(1e-10, x0, o2, 0.0, *((lb, ub) if box is not None else (None, None)))
    with pytest.raises(R.MaxIterReached):
        prox.minimize(RP.GLLQuadratic(1e-4, 10), o2, iters, 50)
    assert len(spg.trace) == len(prox.trace) == iters and o1.calls == o2.calls
    for k in range(iters):
        a, p = spg.trace[k], prox.trace[k]
        for key in ("f", "gnorm", "t", "n_evals", "ls_iters", "s_norm"):
            assert a[key] == p[key], (k, key, a[key], p[key])
        assert spg.trace_x[k].tobytes() == prox.trace_x[k].tobytes(), k
    assert spg.lam == prox.lam


@pytest.mark.parametrize("boxed", [False, True])
def test_closed_form_separable_quadratic(boxed):
    """f = 1/2 sum q_j (x_j - c_j)^2: the minimiser of f + h in the box is clip(soft(c_j, l1_j / q_j)), entry by entry (1-D and convex).  At a
    point that passes rule 2 with tolerance tol, |q_j (x_j - x*_j)| < tol wherever x_j and x*_j have the same sign pattern, so |x - x*| < tol / min q;
    an entry with |c_j| q_j < l1_j - tol cannot be anything but 0.0 there (its measure would be at least l1_j - q_j |c_j| otherwise)."""
    n, tol = 200, 1e-9
    rng = np.random.default_rng(11)
    q = rng.uniform(1.0, 50.0, n)
    c = rng.standard_normal(n)
    l1 = rng.uniform(0.0, 30.0, n)
    l1[::9] = 0.0
    lb, ub = (np.full(n, -0.4), np.full(n, 0.7)) if boxed else (None, None)

    def fn(x):
        return 0.5 * float(np.sum(q * (x - c) ** 2)), q * (x - c)
    soft = np.sign(c) * np.maximum(np.abs(c) - l1 / q, 0.0)
    want = np.clip(soft, lb, ub) if boxed else soft
    must_be_zero = np.abs(c) * q < l1 - 1e-6
    assert 20 < must_be_zero.sum() < n - 20 and not np.any((np.abs(np.abs(c) * q - l1) < 1e-6) & (l1 > 0))
    o = R.CountingOracle(fn)
    s = RP.SpectralProximalGradient(tol, rng.standard_normal(n), o, l1, lb, ub)
    s.minimize(RP.GLLQuadratic(1e-4, 10), o, 2000, 50)  # returns: converged
    assert s.has_converged(fn(s.x))
    assert np.all(s.x[must_be_zero] == 0.0)
    assert np.max(np.abs(s.x - want)) <= tol / q.min()
    if boxed:
        assert np.all(s.x >= lb) and np.all(s.x <= ub) and np.any(s.x == lb) and np.any(s.x == ub)


@pytest.mark.parametrize("kind,shape,ls", PC.WINDOW_CASES)
def test_window_self_check(qo, kind, shape, ls):
    """the family's own: numpy.dot, math.fsum and a reversed-order sum take the same decisions over the window tests/test_gpu_prox.py compares"""
    w = PC.window(kind, shape, ls, qo)
    assert w == PC.WINDOWS[(kind, shape, ls)], w
    assert w >= 20
    a = PC.run_ref(kind, shape, ls, qo)[0]
    assert 0 < np.count_nonzero(a.x) < a.x.size  # the penalty bites: exact zeros and live entries
    if ls == "bt":
        assert any(r["ls_iters"] > 1 for r in a.trace[:w])  # the search's second branch is inside the window


def test_whole_runs_converge():
    """check 9's yardstick: the restatement's own iteration counts, and the zero patterns the GPU run must reproduce"""
    for case in PC.RUN_CASES:
        s, status = PC.run_whole(*case)
        assert status == "ok", case
        n = case[2]
        assert 0 < np.count_nonzero(s.x) < n, case
        assert s.has_converged(PC.run_problem(*case[:3])[0](s.x))
        if case[3]:
            assert s.x.min() == 0.0


# ---- planted faults: each wrong rule is rejected by a comparison these tests and the GPU tests make ----
def _window_rejects(qo, fault, kind, shape, ls):
    clean = PC.run_ref(kind, shape, ls, qo)[0]
    bad = PC.run_ref(kind, shape, ls, qo, faults=(fault,))[0]
    return PC.agree(clean, bad, PC.WINDOWS[(kind, shape, ls)])


@pytest.mark.parametrize("fault", ["tau_without_lambda", "delta_is_gd", "smooth_f_in_ring"])
def test_planted_fault_breaks_a_window(qo, fault):
    """the window comparison (equal counts, t and x to 1e-9, the measure to 1e-7) against the clean restatement"""
    broken = [c for c in PC.WINDOW_CASES if _window_rejects(qo, fault, *c) is not None]
    assert broken, fault


def test_planted_fault_tau_without_lambda_changes_the_direction():
    """... and the direction's bit-for-bit comparison: rule 1 from (x, g, lambda) differs wherever lambda != 1"""
    rng = np.random.default_rng(3)
    x, g, l1 = rng.standard_normal(50), rng.standard_normal(50), np.full(50, 0.3)
    good, _ = RP.prox_direction(x, g, 0.37, l1)
    bad, _ = RP.prox_direction(x, g, 0.37, l1, faults=("tau_without_lambda",))
    assert good.tobytes() != bad.tobytes()


def test_planted_fault_measure_at_zero():
    """the measure's bit-for-bit comparison: at x_j == 0 with |g_j| <= l1_j the entry is stationary, g_j is not its measure; and a run with the
    fault never meets the tolerance on a problem whose solution has zeros"""
    x, g, l1 = np.array([0.0, 0.0, 1.0]), np.array([0.2, -0.9, -0.5]), np.array([0.5, 0.5, 0.5])
    good, bad = RP.measure(x, g, l1), RP.measure(x, g, l1, faults=("measure_at_zero_is_g",))
    assert np.array_equal(good, [0.0, -0.4, 0.0]) and good.tobytes() != bad.tobytes()
    fn, _, _, x0, l1t = PC.tiny_problem()
    big = 100.0 * l1t  # the solution has an entry at exactly 0 whose gradient is not 0
    o = R.CountingOracle(fn)
    s = RP.SpectralProximalGradient(1e-9, x0, o, big, faults=("measure_at_zero_is_g",))
    with pytest.raises(R.MaxIterReached):
        s.minimize(RP.GLLQuadratic(1e-4, 10), o, 200, 50)
    o = R.CountingOracle(fn)
    s = RP.SpectralProximalGradient(1e-9, x0, o, big)
    s.minimize(RP.GLLQuadratic(1e-4, 10), o, 200, 50)
    assert np.any(s.x == 0.0)


def test_planted_fault_h1_from_p():
    """h1 from the prox point p instead of the rounded x + d moves Delta by rounding only: at n = 2, where every sum has one order and the GPU's
    run is the restatement's bit for bit (tests/test_gpu_prox.py::test_tiny_runs_bit_for_bit), it changes the bits of the first search's t"""
    clean, bad = PC.run_tiny(), PC.run_tiny(faults=("h1_from_p",))
    assert clean.trace[0]["ls_iters"] > 1
    assert clean.trace[0]["t"] != bad.trace[0]["t"]
    assert clean.trace[0]["delta"] != bad.trace[0]["delta"]


def test_set_l1_clears_the_ring_and_it_shows():
    """rule 7 on the case tests/test_gpu_prox.py::test_set_l1_between_calls runs: the first search after set_l1 differs between a cleared and a kept ring"""
    cleared, kept = PC.run_restart(True)[1][0], PC.run_restart(False)[1][0]
    assert cleared["ls_iters"] == 2 and kept["ls_iters"] == 1 and kept["t"] == 1.0 and cleared["t"] < 1.0


def test_every_fault_is_covered():
    assert set(RP.FAULTS) == {"tau_without_lambda", "delta_is_gd", "smooth_f_in_ring", "measure_at_zero_is_g", "h1_from_p"}
