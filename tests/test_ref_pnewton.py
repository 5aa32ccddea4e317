"""CPU tests of the restatement tests/ref_pnewton.py: the reference's own two tests, hand-checked cases of ProjectedNewton's three-step
convergence order, and the summation-order self-check that licenses every window tests/test_gpu_pnewton.py compares on the GPU."""
import math

import numpy as np
import pytest

import pnewton_cases as C
import ref_pnewton as RP
import ref_spg as R
import spg_cases as S


def _two_var(gamma):
    h = np.array([[1.0, 0.0], [0.0, gamma]])

    def fn(x):
        return 0.5 * (x[0] ** 2 + gamma * x[1] ** 2), np.array([x[0], gamma * x[1]]), h
    return fn


def test_projected_newton_reference_test():  # projected_newton.rs:147-198
    o = RP.HessianOracle(_two_var(90.0))
    s = RP.ProjectedNewton(1e-6, [180.0, 152.0], [-np.inf, -np.inf], [np.inf, np.inf])
    s.minimize(R.GLLQuadratic(1e-4, 15), o, 10000, 1000)  # Ok(())
    assert s.has_converged(o(s.x))
    assert s.k == 1 and np.max(np.abs(s.x)) <= 1e-12  # one Newton step on a quadratic (sqrt(90)^2 is not 90: a last-bit residue)
    assert s.ended_by == "projected_gradient"


def test_spectral_projected_newton_reference_test():  # spn.rs:155-210
    o = RP.HessianOracle(_two_var(1e9))
    lb, ub = np.array([-1.0, 47.0]), np.array([np.inf, np.inf])
    s = RP.SpectralProjectedNewton(1e-12, [180.0, 152.0], o, lb, ub)
    s.minimize(R.GLLQuadratic(1e-4, 10), o, 10000, 1000)  # Ok(())
    assert np.all(s.x >= lb) and np.all(s.x <= ub)
    assert s.has_converged(o(s.x))
    assert s.x[1] == 47.0


def test_nalgebra_order_cholesky_against_lapack():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 5, 8):
        a = rng.standard_normal((n, n))
        h = a @ a.T + n * np.eye(n)
        g = rng.standard_normal(n)
        z = RP._nalgebra_solve(RP._nalgebra_cholesky(h), g, np.dot)
        assert np.allclose(z, np.linalg.solve(h, g), rtol=1e-12, atol=0)
    # only the lower triangle is read
    h = np.array([[4.0, 99.0], [1.0, 3.0]])
    assert np.allclose(RP.CholeskySolve()(h, np.array([1.0, 2.0])), np.linalg.solve(np.array([[4.0, 1.0], [1.0, 3.0]]), [1.0, 2.0]))
    with pytest.raises(RP.NotPositiveDefinite):
        RP.CholeskySolve()(np.array([[1.0, 0.0], [0.0, -1.0]]), np.ones(2))
    big = rng.standard_normal((40, 40))
    big = big @ big.T - 50.0 * np.eye(40)
    with pytest.raises(RP.NotPositiveDefinite):
        RP.CholeskySolve()(big, np.ones(40))


def test_convergence_order_by_hand():
    """projected_newton.rs:95-110, three hand-checked cases on f = 1/2 x'x (H = I, so d = P(0) - x)."""
    eye = np.eye(2)
    fn = lambda x: (0.5 * float(x @ x), x.copy(), eye)  # noqa: E731
    inf = np.array([np.inf, np.inf])
    # (1) nothing recorded yet: the projected gradient decides; x0 = 0 converges with k = 0 and s_norm None
    s = RP.ProjectedNewton(1e-8, [0.0, 0.0], -inf, inf)
    s.minimize(R.GLLQuadratic(1e-4, 10), RP.HessianOracle(fn), 10, 10)
    assert (s.k, s.ended_by, s.s_norm) == (0, "projected_gradient", None)
    # (2) one full step to 0: s_norm = ||x0|| = 5, y_norm = 5, then g = 0: ends by the projected gradient at k = 1
    s = RP.ProjectedNewton(1e-8, [3.0, 4.0], -inf, inf)
    s.minimize(R.GLLQuadratic(1e-4, 10), RP.HessianOracle(fn), 10, 10)
    assert (s.k, s.ended_by, s.s_norm, s.y_norm) == (1, "projected_gradient", 5.0, 5.0)
    # (3) the box stops the step at x = (1, 1): iteration 2 has d = 0, so s_norm = 0 < tol ends the run at the third loop top while the
    # projected gradient there is (0, 0) too -- s_norm is tested FIRST
    s = RP.ProjectedNewton(1e-8, [3.0, 4.0], np.array([1.0, 1.0]), inf)
    s.minimize(R.GLLQuadratic(1e-4, 10), RP.HessianOracle(fn), 10, 10)
    assert np.array_equal(s.x, [1.0, 1.0]) and s.ended_by == "projected_gradient" and s.k == 1
    # (4) s_norm below tol with a projected gradient that is NOT: a tolerance larger than the step ends the run by s_norm
    s = RP.ProjectedNewton(10.0, [3.0, 40.0], -inf, inf)
    s.s_norm, s.y_norm = 5.0, 50.0
    assert s.has_converged(RP.Eval(0.0, np.array([3.0, 40.0]), eye)) and s.ended_by == "s_norm"
    # (5) y_norm second
    s.s_norm, s.y_norm = 50.0, 5.0
    assert s.has_converged(RP.Eval(0.0, np.array([3.0, 40.0]), eye)) and s.ended_by == "y_norm"
    s.s_norm, s.y_norm = 50.0, 50.0
    assert not s.has_converged(RP.Eval(0.0, np.array([3.0, 40.0]), eye))


def _self_check(solver, fn, x0, lb, ub):
    a, oa, sa = C.run_ref(solver, fn, x0, lb, ub, C.WINDOW, solve=RP.CholeskySolve(np.dot), dot=np.dot)
    b, ob, sb = C.run_ref(solver, fn, x0, lb, ub, C.WINDOW, solve=RP.LUSolve(), dot=R.fsum_dot)
    assert sa == sb and oa.calls == ob.calls and len(a.trace) == len(b.trace) >= 1, (sa, sb, oa.calls, ob.calls, len(a.trace), len(b.trace))
    spread = 0.0
    for ra, rb, xa, xb in zip(a.trace, b.trace, a.trace_x, b.trace_x):
        assert ra["n_evals"] == rb["n_evals"] and ra["ls_iters"] == rb["ls_iters"]
        spread = max(spread, float(np.linalg.norm(xa - xb) / max(1.0, np.linalg.norm(xa))), abs(ra["t"] - rb["t"]) / abs(ra["t"]))
    print(f"self-check {solver}: iterations={len(a.trace)} status={sa} spread={spread:.3e}")
    assert spread <= 1e-10, spread  # the project's factor 10 inside the 1e-9 the GPU tests allow
    return a, sa


@pytest.mark.parametrize("solver,n,box", C.QUAD_CASES)
def test_summation_order_self_check_quadratic(qo, solver, n, box):
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, box)
    a, status = _self_check(solver, RP.quadratic_fn(q, b), x0, lb, ub)
    if solver == "spn":
        assert status == "max_iter" and len(a.trace) == C.WINDOW
    else:  # ends after 1-2 iterations: by the gradient test in the infinite box, by s_norm in +-0.05
        assert status == "ok" and 1 <= len(a.trace) <= 2
        assert a.ended_by == ("projected_gradient" if math.isinf(box) else "s_norm")


@pytest.mark.parametrize("solver,box", C.LSE_CASES)
def test_summation_order_self_check_logsumexp(solver, box):
    a_, c_, mu, x0, _, _ = S.lse_problem()
    n = x0.size
    lb, ub = S.bounds(n, box)
    a, status = _self_check(solver, C.lse_hess_fn(a_, c_, mu), x0, lb, ub)
    if solver == "spn":
        assert len(a.trace) == C.WINDOW
    else:
        assert len(a.trace) == (14 if box == 0.3 else C.WINDOW)


def test_self_check_synthetic_4096(qo):
    q, b, x0, _ = S.problem(qo, C.BIG_N)
    for box in C.BOXES:
        lb, ub = S.bounds(C.BIG_N, box)
        for solver in C.SOLVERS:
            _self_check(solver, RP.quadratic_fn(q, b), x0, lb, ub)
