"""CPU tests of tests/ref_spg.py, the restatement the GPU solvers QN_SPG / QN_PROJECTED_GRADIENT are checked against: what the reference
itself pins (spg.rs:151-204, projected_gradient_descent.rs:114-165: Ok and converged -- it asserts no values), hand-checkable cases of
GLLQuadratic, and the summation-order self-check that licenses the windows of tests/test_gpu_spg.py."""
import math

import numpy as np
import pytest

import ref_spg as R
import spg_cases as S


def _two_var(gamma):
    def fn(x):
        return 0.5 * (x[0] ** 2 + gamma * x[1] ** 2), np.array([x[0], gamma * x[1]])
    return fn


def test_spg_reference_test():  # spg.rs:151-204
    o = R.CountingOracle(_two_var(1e9))
    lb, ub = np.array([-1.0, 47.0]), np.array([np.inf, np.inf])
    s = R.SpectralProjectedGradient(1e-12, [180.0, 152.0], o, lb, ub)
    s.minimize(R.GLLQuadratic(1e-4, 10), o, 10000, 1000)  # Ok(()): raises otherwise
    assert np.all(s.x >= lb) and np.all(s.x <= ub)
    assert s.has_converged(o(s.x))


def test_pgd_reference_test():  # projected_gradient_descent.rs:114-165
    o = R.CountingOracle(_two_var(999.0))
    lb, ub = np.array([-np.inf, -np.inf]), np.array([np.inf, np.inf])
    s = R.ProjectedGradientDescent(1e-6, [180.0, 152.0], lb, ub)
    s.minimize(R.BackTrackingB(1e-4, 0.5, lb, ub), o, 10000, 1000)
    assert np.all(s.x >= lb) and np.all(s.x <= ub)
    assert s.has_converged(o(s.x))


def _scripted(values):
    it = iter(values)
    return R.CountingOracle(lambda x: (next(it), np.zeros_like(x)))


def test_gll_m1_is_monotone_armijo():
    # m = 1: f_previous holds f_k alone, so f_max = f_k and the test is backtracking.rs's Armijo test (gll_quadratic.rs:5)
    x, g, d = np.array([0.0]), np.array([-1.0]), np.array([1.0])
    ls = R.GLLQuadratic(1e-4, 1)
    for f_k in (5.0, 3.0, 4.0):  # a larger f_k after a smaller one: a longer look-back would keep 5.0
        t = ls.compute_step_len(x, (f_k, g), d, _scripted([f_k - 1.0]), 10)
        assert t == 1.0 and ls.f_previous == [f_k] and ls.f_max() == f_k
    # f_kp1 = f_k + 1 fails Armijo against f_k with m = 1, but passes against the history's maximum with m = 2
    assert R.GLLQuadratic(1e-4, 1).compute_step_len(x, (0.0, g), d, _scripted([1.0, -1.0]), 10) != 1.0
    ls2 = R.GLLQuadratic(1e-4, 2)
    ls2.append_new_f(10.0)
    assert ls2.compute_step_len(x, (0.0, g), d, _scripted([1.0]), 10) == 1.0


def test_gll_ring_drops_the_oldest():
    ls = R.GLLQuadratic(1e-4, 3)
    for f in (1.0, 9.0, 2.0, 3.0, 4.0):
        ls.append_new_f(f)
    assert ls.f_previous == [2.0, 3.0, 4.0] and ls.f_max() == 4.0


def test_gll_three_branches_by_hand():
    x, g, d = np.array([0.0]), np.array([-1.0]), np.array([1.0])  # g.d = -1, f_k = 0
    # t = 1, f = 0.5: t_tmp = -0.5 * 1 * 1 * -1 / (0.5 - 0 + 1) = 1/3, inside (0.1, 0.9): taken as it is; then f = -1 passes
    ls = R.GLLQuadratic(1e-4, 10)
    t = ls.compute_step_len(x, (0.0, g), d, _scripted([0.5, -1.0]), 10)
    assert ls.branches == ["interp", "accept"] and t == 0.5 / 1.5
    # t = 1, f = 10: t_tmp = 0.5 / 11 < sigma1: halved -> 0.25 / 11; that t <= 0.1 and f = 10 again: t *= 0.5; then accepted
    ls = R.GLLQuadratic(1e-4, 10)
    t = ls.compute_step_len(x, (0.0, g), d, _scripted([10.0, 10.0, -1.0]), 10)
    assert ls.branches == ["half_interp", "halve", "accept"]
    assert t == (0.5 / 11.0) * 0.5 * 0.5
    # the cap: every trial fails, the last t is returned unevaluated
    ls = R.GLLQuadratic(1e-4, 10)
    t = ls.compute_step_len(x, (0.0, g), d, _scripted([10.0, 10.0]), 2)
    assert ls.trials == 2 and t == (0.5 / 11.0) * 0.5 * 0.5
    # a NaN f is not repaired: it fails Armijo and makes t_tmp NaN
    ls = R.GLLQuadratic(1e-4, 10)
    assert math.isnan(ls.compute_step_len(x, (0.0, g), d, _scripted([float("nan")]), 1))


@pytest.mark.parametrize("solver,n,box", S.CASES + [(s, S.BIG_N, b) for s in S.SOLVERS for b in S.BOXES])
def test_summation_order_self_check(qo, solver, n, box):
    """The restatement with numpy.dot and with math.fsum as the dot product: equal decisions, iterates within 1e-10 relative over the
    window -- a factor 10 inside the 1e-9 the GPU tests allow for the GPU's own (third) summation order."""
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, box)
    fn = R.quadratic_fn(q, b)
    a, oa = S.run_ref(solver, fn, x0, lb, ub, S.WINDOW, dot=np.dot)
    c, oc = S.run_ref(solver, fn, x0, lb, ub, S.WINDOW, dot=R.fsum_dot)
    assert len(a.trace) == len(c.trace) == S.WINDOW
    assert [r["n_evals"] for r in a.trace] == [r["n_evals"] for r in c.trace]
    assert [r["ls_iters"] for r in a.trace] == [r["ls_iters"] for r in c.trace]
    worst = 0.0
    for k in range(S.WINDOW):
        worst = max(worst, np.linalg.norm(a.trace_x[k] - c.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k])))
        assert abs(a.trace[k]["t"] - c.trace[k]["t"]) <= 1e-10 * abs(a.trace[k]["t"])
    print(f"{solver} n={n} box={box}: worst relative iterate difference {worst:.2e}, calls {oa.calls}")
    assert worst <= 1e-10


def _self_check(solver, fn, x0, lb, ub, label):
    a, oa = S.run_ref(solver, fn, x0, lb, ub, S.WINDOW, dot=np.dot)
    c, _ = S.run_ref(solver, fn, x0, lb, ub, S.WINDOW, dot=R.fsum_dot)
    assert len(a.trace) == len(c.trace) == S.WINDOW
    assert [r["n_evals"] for r in a.trace] == [r["n_evals"] for r in c.trace]
    assert [r["ls_iters"] for r in a.trace] == [r["ls_iters"] for r in c.trace]
    worst = 0.0
    for k in range(S.WINDOW):
        worst = max(worst, np.linalg.norm(a.trace_x[k] - c.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k])))
        assert abs(a.trace[k]["t"] - c.trace[k]["t"]) <= 1e-10 * abs(a.trace[k]["t"])
    print(f"{label} {solver}: worst relative iterate difference {worst:.2e}, calls {oa.calls}")
    assert worst <= 1e-10


@pytest.mark.parametrize("solver", S.SOLVERS)
def test_summation_order_self_check_device_closure_problem(solver):
    """The same self-check on the double-well chain the GPU tests run through a device closure: the 30-iteration window holds."""
    a, c, x0, lb, ub = S.chain_problem()
    _self_check(solver, S.chain_fn(a, c), x0, lb, ub, "chain")


def test_summation_order_self_check_logsumexp_problem():
    """... and on the small log-sum-exp problem of the GPU test."""
    a, c, mu, x0, lb, ub = S.lse_problem()
    _self_check("spg_gll", S.lse_fn(a, c, mu), x0, lb, ub, "logsumexp")


def test_builders_are_plain_data(qn):
    """The builders are plain data: kind, m and the sigmas travel in the existing fields of qn_linesearch."""
    ls = qn.GLLQuadratic(1e-4, 10).with_sigmas(0.2, 0.8)
    assert ls.s.kind == 4 and ls.s._pad == 10 and ls.s.c1 == 1e-4 and ls.s.delta_min == 0.2 and ls.s.delta_max == 0.8
    assert qn.GLLQuadratic.new(1e-4, 3).s.delta_min == 0.1 and qn.GLLQuadratic.new(1e-4, 3).s.delta_max == 0.9
