"""CPU tests of tests/ref_steepest.py, the restatement the GPU solvers QN_PNORM_DESCENT / QN_COORDINATE_DESCENT and QN_LS_NO_SEARCH are compared
with (tests/test_gpu_steepest.py): it reproduces the assertions of the reference's own four tests with the iteration and oracle-call counts the
restatement gives, pins CoordinateDescent's fold as written (the sign quirk, first-index ties, NaN entries), and licenses every window of
tests/steepest_cases.py -- the measured order spreads are printed (-s) and recorded there, where the GPU tolerances come from."""
import math

import numpy as np
import pytest

import ref_steepest as R
import steepest_cases as SC


@pytest.mark.parametrize("name,solver,ls,iters,calls", SC.REFERENCE_TESTS)
def test_reference_tests_assertions(name, solver, ls, iters, calls):
    """pnorm_descent.rs:92-140,143-193, coordinate_descent.rs:102-148,151-198: minimize(.., 1000, 100).unwrap(); assert |f| < 1e-6"""
    s, o, status = SC.run_ref(solver, SC.two_var(), SC.X0_2D.copy(), ls, 1000, SC.INVERSE_P_2D, max_ls=100)
    assert status == "ok"
    f, g = SC.two_var()(s.x)
    assert abs(f - 0.0) < 1e-6
    assert s.has_converged((f, g))
    print(f"{name}: iterations = {s.k}  oracle calls = {o.calls}  distinct points = {o.evals}")
    assert (s.k, o.calls) == (iters, calls)


def test_pnorm_direction_is_minus_p_times_g_rows_not_columns():
    p = np.array([[1.0, 2.0], [0.0, 3.0]])
    s = R.PnormDescent(1e-12, np.zeros(2), p)
    assert np.array_equal(s.compute_direction((0.0, np.array([1.0, 10.0]))), np.array([-21.0, -30.0]))
    assert np.array_equal(R.PnormDescent(1e-12, np.zeros(2), p, "fsum").compute_direction((0.0, np.array([1.0, 10.0]))), np.array([-21.0, -30.0]))


def test_coordinate_descent_sign_quirk():
    """coordinate_descent.rs:43: `-max_value.signum()` of a MAGNITUDE is -1.0 whatever the sign of the gradient's entry.  From (-3, 1) on the
    gamma = 90 problem the first direction is -e_1 (g = (-3, 90): descent, t = 1 lands on x_1 = 0) and the second is -e_0 although g_0 = -3 < 0: an
    ASCENT direction.  BackTracking(1e-4, 0.5) with max_iter_line_search = 100 then shrinks t until x_0 - t rounds back to x_0 = -3, where
    f1 - f_k = 0 <= c1 t (g.d) holds with g.d = +3: it returns t = 0.5**52 (half an ulp of 3) and the iterate does not move.  (With an |x_0| small
    enough that x_0 - t stays distinct down to 0.5**100 the search exhausts its 100 iterations and returns 0.5**100: the second case.)"""
    s, o, status = SC.run_ref("cd", SC.two_var(), np.array([-3.0, 1.0]), "bt", 3, max_ls=100)
    assert status == "max_iter"
    assert [d.tolist() for d in s.trace_d] == [[0.0, -1.0], [-1.0, 0.0], [-1.0, 0.0]]
    assert [r["t"] for r in s.trace] == [1.0, 0.5 ** 52, 0.5 ** 52]
    assert np.array_equal(np.array(s.trace_x), np.array([[-3.0, 0.0]] * 3))
    s, o, status = SC.run_ref("cd", SC.two_var(), np.array([-(0.5 ** 60), 1.0]), "bt", 2, tol=1e-30, max_ls=100)
    assert [d.tolist() for d in s.trace_d] == [[0.0, -1.0], [-1.0, 0.0]]
    assert [r["t"] for r in s.trace] == [1.0, 0.5 ** 100]
    assert s.trace[1]["n_evals"] == 1 + 100  # the loop-top call and max_iter_line_search trials


def test_coordinate_fold_first_index_ties_and_nan():
    nan = float("nan")
    assert R.coordinate_fold(np.array([1.0, -4.0, 4.0, -4.0])) == (1, 4.0)          # strict >: the FIRST of the largest magnitudes
    assert R.coordinate_fold(np.array([nan, 2.0, nan, -2.0])) == (1, 2.0)           # a NaN never wins
    assert R.coordinate_fold(np.array([nan, nan])) == (0, 0.0)                      # ... and nothing above 0.0 leaves the fold's start
    assert R.coordinate_fold(np.zeros(5)) == (0, 0.0)
    assert R.coordinate_fold(np.array([-0.0, 0.0, float("inf"), float("inf")])) == (2, float("inf"))
    s = R.CoordinateDescent(1e-12, np.zeros(3))
    assert np.array_equal(s.compute_direction((0.0, np.zeros(3))), np.array([-1.0, 0.0, 0.0]))       # -e_0: 0.0f64.signum() is 1.0
    assert np.array_equal(s.compute_direction((0.0, np.array([nan, nan, nan]))), np.array([-1.0, 0.0, 0.0]))
    assert np.array_equal(s.compute_direction((0.0, np.array([1.0, -7.0, 7.0]))), np.array([0.0, -1.0, 0.0]))
    assert R.inf_norm(np.array([nan, -3.0, 2.0])) == 3.0 and R.inf_norm(np.array([nan, nan])) == -math.inf
    assert s.has_converged((0.0, np.array([nan, nan, nan])))   # -inf < tol


def test_nosearch_takes_the_full_step_without_a_call():
    fn = SC.two_var(2.0)
    s, o, status = SC.run_ref("gd", fn, np.array([1.0, 1.0]), "none", 3)
    assert status == "max_iter" and o.calls == 3 and [r["t"] for r in s.trace] == [1.0] * 3
    assert np.array_equal(np.array(s.trace_x), np.array([[0.0, -1.0], [0.0, 1.0], [0.0, -1.0]]))  # x + d, d = -g


@pytest.mark.parametrize("name", list(SC.WINDOWS))
def test_window_is_licensed(qo, name):
    w = SC.WINDOWS[name]
    pr, s, o, status = SC.window_ref(name, qo)
    assert status == "max_iter" and s.k == w["K"]
    assert np.all(np.isfinite(np.array(s.trace_x))) and all(np.isfinite(r["f"]) for r in s.trace)
    asym = float(np.max(np.abs(pr["p"] - pr["p"].T)))
    assert asym > 1e-6 * float(np.max(np.abs(pr["p"]))), asym       # inverse_p is clearly not symmetric
    assert all(r["f"] > s.trace[i + 1]["f"] for i, r in enumerate(s.trace[:-1]))  # a descent method on it
    spread = SC.spread_of(pr, w)
    print(f"{name}: K = {w['K']}  order spread = {spread:.3e}  recorded = {w['spread']:.3e}  GPU tolerance = {SC.tolerance(w):.3e}  calls = {o.calls} evals = {o.evals}")
    assert spread <= w["spread"] < SC.SPREAD_CAP and SC.tolerance(w) <= SC.MARGIN * SC.SPREAD_CAP
