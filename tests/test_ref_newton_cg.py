"""CPU tests of the restatement tests/ref_newton_cg.py, and the self-checks that license every window tests/test_gpu_newton_cg.py compares on the
GPU (the method of tests/test_ref_cg.py): each case runs with numpy.dot, with math.fsum of the products and with every dot product summed in
reversed order, and twice with evaluations and Hessian-vector products moved by a few ulp (newton_cg_cases.licence); a window ends where x or t
differ by more than the licence or any decision -- t, n_evals, the inner count j_k, an exit reason -- differs."""
import math

import numpy as np
import pytest

import newton_cg_cases as NC
import ref_newton_cg as RN
import spg_cases as S


@pytest.mark.parametrize("m,n,ls", NC.CASES)
def test_self_check_window(m, n, ls):
    w, worst, length = NC.licence(m, n, ls)
    a, _, status = NC.ref_case(m, n, ls)
    print(f"self-check {(m, n, ls)}: window={w} of {length} ({status}) spread={worst:.3e} inner={a.inner} why={sorted(set(a.why))}")
    # (the floor rule judges iteration k by f_{k+1}, which the trace holds for all but the last iteration: "the whole run" is length - 1)
    assert w >= min(NC.MIN_WINDOW, length - 1), (w, length)
    assert worst <= NC.LICENCE, worst


@pytest.mark.parametrize("m,n", NC.CONVERGENCE)
def test_restatement_converges_as_the_trial_did(m, n):
    """BackTracking(1e-4, 0.5), tol 1e-7 from x0: the restatement ends OK; the first trial is accepted in the last iterations; ||g||_inf recomputed"""
    a, o, status = NC.ref_case(m, n, "bt")
    assert status == "ok" and 8 <= a.k <= 20, (status, a.k)
    am, c, mu, _ = NC.problem(m, n)
    g = S.lse_fn(am, c, mu)(a.x)[1]
    assert float(np.max(np.abs(g))) < NC.TOL
    assert a.trace[-1]["t"] == 1.0 and a.neg_curv == 0 and a.fallbacks == 0
    assert a.hv_passes == sum(a.inner)
    print(f"({m}, {n}): {a.k} outer iterations, inner {a.inner} ({sum(a.inner)} in all), {o.calls} evaluations")


def test_from_a_spread_start_every_step_is_one():
    for m, n in NC.CONVERGENCE:
        am, c, mu, x0 = NC.problem(m, n)
        s = RN.NewtonCG(NC.TOL, 0.01 * x0, RN.lse_hess_vec_at(am, c, mu))
        s.minimize(NC.line_search("bt"), NC.R.CountingOracle(S.lse_fn(am, c, mu)), NC.ITERS, NC.MAX_LS)
        assert all(r["t"] == 1.0 for r in s.trace) and s.k <= 10, (m, n, s.k)


def test_max_inner_caps_the_loop():
    a, _, status = NC.run_ref(96, 64, "bt", max_inner=2)
    assert max(a.inner) == 2 and "cap" in a.why and all(j <= 2 for j in a.inner)


def test_negative_curvature_takes_rule_4_at_j_0():
    """(3, 5) with mu = NEG_MU: the first direction's kappa = g'Hg is negative, z = g, d = -g"""
    a, _, _ = NC.run_ref(3, 5, "bt", iters=3, mu=NC.NEG_MU)
    am, c, _, x0 = NC.problem(3, 5)
    g0 = S.lse_fn(am, c, NC.NEG_MU)(x0)[1]
    assert a.why[0] == "negcurv" and a.inner[0] == 0 and a.neg_curv >= 1
    assert np.array_equal(a.directions[0], -g0)
    q = RN.lse_hess_vec_at(am, c, NC.NEG_MU)(x0)(g0)
    assert float(g0 @ q) < -1e-3 * float(g0 @ g0)  # well clear of zero: no summation order changes the branch


def test_rules_by_hand_on_a_diagonal_hessian():
    """H = diag(h) through a product of the test's own: CG's first step is alpha = g.g / g'Hg; with eta_max tiny the loop runs to n steps and
    solves the system; a product that returns -v takes rule 4 at j = 0"""
    h = np.array([1.0, 2.0, 4.0])
    g = np.array([1.0, -1.0, 0.5])
    s = RN.NewtonCG(1e-12, np.zeros(3), lambda x: (lambda v: h * v), eta_max=1e-12, max_inner=3)
    d = s.compute_direction((0.0, g))
    assert s.inner == [3] and np.allclose(d, -g / h, rtol=1e-12, atol=0.0)
    s1 = RN.NewtonCG(1e-12, np.zeros(3), lambda x: (lambda v: h * v), eta_max=0.999, max_inner=1)
    d1 = s1.compute_direction((0.0, g))
    alpha = float(g @ g) / float(g @ (h * g))
    assert s1.inner == [1] and np.array_equal(d1, -(alpha * g))
    s2 = RN.NewtonCG(1e-12, np.zeros(3), lambda x: (lambda v: -v))
    assert np.array_equal(s2.compute_direction((0.0, g)), -g) and s2.why == ["negcurv"] and s2.neg_curv == 1 and s2.fallbacks == 0
    eta = math.sqrt(math.sqrt(float(g @ g)))
    assert eta > 0.5  # (the default cap 0.5 is the forcing term here)


def test_two_calls_are_one():
    one, _, _ = NC.run_ref(96, 64, "bt", iters=8)
    two, _, _ = NC.run_ref(96, 64, "bt", iters=4)
    NC.run_ref(96, 64, "bt", iters=4, solver=two)
    assert np.array_equal(one.x, two.x) and one.inner == two.inner
