"""CPU tests of tests/ref_exact.py, the restatement the ExactQuadratic search (QN_LS_EXACT_QUADRATIC) is compared with on the GPU, and the licences of
tests/exact_cases.py's windows: every case runs with numpy.dot, with math.fsum and with every sum reversed; a window is at least 8 iterations, or the
whole run where every order converges sooner.  No GPU, no library."""
import numpy as np
import pytest

import exact_cases as EC
import ref_exact as RE
import sparse_cases as SC


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_window_is_licensed(case):
    w, whole_run, worst = EC.licence(case)
    assert w >= EC.MIN_WINDOW or whole_run, (case, w, whole_run)
    assert worst <= EC.LICENCE


def test_the_rule_was_not_shortened_by_the_replacement():
    """what exact_cases.py replaced (ProjectedLBFGS at n = 7) does fall under the rule, and the case kept for the error path ends the same way in every order"""
    w, whole_run, _ = EC.licence(EC.NOT_DESCENT_CASE)
    a, _, _, status = EC.ref_case(EC.NOT_DESCENT_CASE)
    assert w < EC.MIN_WINDOW and not whole_run and status == "not_descent"
    assert w == len(a.trace)  # ... but the three orders agree on every iteration it has
    for order in ("fsum", "reversed"):
        s, _, _, st = EC.run_ref(EC.NOT_DESCENT_CASE, order=order)
        assert st == "not_descent" and len(s.trace) == len(a.trace)


def test_the_search_is_the_exact_minimiser_and_the_recurrence_is_the_gradient():
    """on a quadratic the step zeroes the directional derivative, and g + t Q d is the gradient at x + t d, to rounding"""
    n = 7
    csr, b, x0 = SC.tri(n), SC.rhs(n), SC.start(n)
    fn = SC.quadratic_fn(csr, b)
    o = RE.ExactOracle(fn, lambda v: SC.matvec(csr, v), 0)
    ls = RE.ExactQuadratic(o)
    f0, g0 = o(x0)
    d = -g0
    t = ls.compute_step_len(x0, (f0, g0), d, o, 0)
    xt, f_t, gt = o.memo
    f_true, g_true = fn(xt)
    assert o.evals == 1 and o.passes == 1 and not o.g_true
    assert abs(float(g_true @ d)) <= 1e-14 * float(np.abs(g_true) @ np.abs(d) + np.abs(g0) @ np.abs(d))
    assert np.max(np.abs(gt - g_true)) <= 1e-14 * np.max(np.abs(g0))
    assert abs(f_t - f_true) <= 1e-14 * max(1.0, abs(f0))
    assert o(xt)[1] is gt and o.evals == 1  # the accepted point's evaluation is handed out, not computed again
    with pytest.raises(RE.NotDescent):
        ls.compute_step_len(x0, (f0, g0), g0, o, 0)
    neg = SC.from_triplets(3, [0, 1, 2], [0, 1, 2], [1.0, -2.0, 1.0])
    o2 = RE.ExactOracle(SC.quadratic_fn(neg, np.ones(3)), lambda v: SC.matvec(neg, v), 1)
    x = np.array([0.0, 5.0, 0.0])
    f, g = o2(x)
    with pytest.raises(RE.NonPositiveCurvature):
        RE.ExactQuadratic(o2).compute_step_len(x, (f, g), -g, o2, 0)


@pytest.mark.parametrize("r", EC.REFRESH)
def test_cg_terminates_in_n_iterations_and_counts(r):
    """linear conjugate gradients at n = 7: about 7 iterations; the objective's evaluations follow the refresh rule"""
    s, ls, o, status = EC.ref_case(("cg-fr", "tri", 7, r))
    it = len(s.trace)
    assert status == "ok" and 6 <= it <= 8
    assert o.passes == it
    if r == 1:
        assert o.evals == it + 1 and o.forced == 0
    if r == 0:
        assert o.evals == 1 + o.forced and o.forced >= 1  # the last gradient was the recurrence's: a true one ended the run
    if r == 3:
        assert o.evals == 1 + it // 3 + o.forced


def test_the_three_orders_agree_on_the_iteration_counts():
    counts = {order: EC.laplacian_cg(order) for order in EC.ORDERS}
    its = [c[0] for c in counts.values()]
    print("laplacian 64 x 64, NonlinearCG(fr) + ExactQuadratic(0), tol 1e-8:", counts)
    assert all(c[1] == "ok" and c[2] >= 1 for c in counts.values())
    assert max(its) - min(its) <= 2
    for order in ("fsum", "reversed"):
        s, _, _, st = EC.run_ref(("cg-fr", "tri", 2050, 0), iters=400, order=order)
        a, _, _, sa = EC.run_ref(("cg-fr", "tri", 2050, 0), iters=400)
        assert st == sa == "ok" and abs(len(s.trace) - len(a.trace)) <= 2


def test_convergence_confirmation_case():
    """the tolerance lies between the recurrence gradient and the true one: the test passes on the first, the objective's evaluation refuses, the run
    goes on -- and, restarted from true gradients, ends a few iterations later on a true gradient under the tolerance"""
    n = EC.CONFIRM_CASE[2]
    fn = SC.quadratic_fn(EC.matrix("tri", n), SC.rhs(n))
    for order in EC.ORDERS:
        z, _, _, _ = EC.run_ref(EC.CONFIRM_CASE, iters=EC.CONFIRM_CAP, order=order, tol=0.0)  # without a tolerance: where the recurrence first passes
        first = next(k for k, rec in enumerate(z.trace) if rec["gnorm"] < EC.CONFIRM_TOL)
        assert first == EC.CONFIRM_FIRST_PASS
        true_there = float(np.max(np.abs(fn(z.trace_x[first - 1])[1])))
        assert true_there > 4.0 * EC.CONFIRM_TOL, (order, true_there)  # ... and the true gradient there does not
        s, _, o, status = EC.confirm_ref(order)
        print(f"confirmation {order}: first pass at {first}, true gradient there {true_there:.2e}, run {status} after {len(s.trace)} iterations, {o.forced} forced")
        assert o.forced >= 1 and len(s.trace) > first, (order, status, len(s.trace), o.forced)
        if status == "ok":
            assert float(np.max(np.abs(fn(s.x)[1]))) < EC.CONFIRM_TOL
