"""CPU tests of the restatement tests/ref_wolfe.py (MINPACK-2 dcsrch / dcstep behind `compute_step_len`), and the self-checks that license every
window tests/test_gpu_wolfe.py compares on the GPU, by the method of tests/test_ref_lbfgs.py: each case runs with numpy.dot, with math.fsum of
the products and with the reversed summation order (L-BFGS also with the compact form); the window is where the runs take the same decisions
(n_evals, ls_iters, ls_cases, updated), agree to 1e-11 in x and t -- a factor of 100 inside the GPU tests' 1e-9 -- and stay above
lbfgs_cases.above_f_floor."""
import math

import numpy as np
import pytest

import ref_spg as R
import ref_wolfe as RW
import wolfe_cases as W

ALL = W.CASES + W.BOX_CASES
EPS = float(np.finfo(np.float64).eps)


def _searches(case):
    _, ls, _, _ = W.ref_case(case)
    return ls.history[:W.window(case)]


def test_step_for_step_against_scipy_dcsrch():
    """every search of every licensed window, replayed through scipy's transcription of the same Fortran: the same trial steps bit for bit and the
    same verdict.  (scipy is the independent statement; only finite trials -- the non-finite rule is this project's own.)"""
    dc = pytest.importorskip("scipy.optimize._dcsrch")
    n = 0
    for case in ALL:
        kw = dict(case[5]) if len(case) > 5 else {}
        for h in _searches(case):
            d = dc.DCSRCH(None, None, kw.get("c1", 1e-4), kw.get("c2", 0.9), kw.get("xtol", 0.1), kw.get("t_min", 0.0), h["stpmax"])
            stp0 = min(max(1.0, kw.get("t_min", 0.0)), h["stpmax"])
            with np.errstate(all="ignore"):
                stp, _, _, task = d._iterate(stp0, h["finit"], h["ginit"], b"START")
                assert task == b"FG"
                for t, f_t, dphi in h["steps"]:
                    assert task == b"FG" and float(stp) == t, (case, h["steps"], stp)
                    stp, _, _, task = d._iterate(t, f_t, dphi, task)
                    n += 1
            if h["evaluated"]:
                assert task.decode().startswith(h["task"][:12]), (task, h["task"])
                assert float(stp) == h["t"]
            else:
                assert task == b"FG" and float(stp) == h["t"]
    assert n > 300


def test_wolfe_inequalities_on_every_returned_step():
    """sufficient decrease and strong curvature at every step a search returned as converged, the directional derivatives recomputed in longdouble
    (f is the function's own value at the float64 trial point); a search that ended on stp = stpmax: sufficient decrease and phi' <= c1 phi'(0)"""
    ends = set()
    for case in ALL:
        kw = dict(case[5]) if len(case) > 5 else {}
        c1, c2 = kw.get("c1", 1e-4), kw.get("c2", 0.9)
        fn = W.problem(case[1], case[2])[0]
        for h in _searches(case):
            assert h["evaluated"], (case, h["steps"])
            ends.add(h["task"])
            d = h["d"].astype(np.longdouble)
            gd = float(np.sum(h["g_k"].astype(np.longdouble) * d))
            t = h["t"]
            f_t, g_t = fn(h["x_k"] + t * h["d"])[:2]
            dphi = float(np.sum(np.asarray(g_t).astype(np.longdouble) * d))
            slack = 64 * EPS * max(1.0, abs(h["finit"]))
            gslack = 1e-12 * float(np.sum(np.abs(np.asarray(g_t) * h["d"]))) + 1e-300
            assert gd < 0.0
            assert f_t <= h["finit"] + c1 * t * gd + slack, (case, h["steps"])
            if h["task"] == "CONVERGENCE":
                assert abs(dphi) <= c2 * abs(gd) + gslack, (case, dphi, gd)
            else:
                assert h["task"] == "WARNING: STP = STPMAX" and t == h["stpmax"] and dphi <= c1 * gd + gslack, (case, h["task"])
    assert ends == {"CONVERGENCE", "WARNING: STP = STPMAX"}


@pytest.mark.parametrize("case", ALL, ids=str)
def test_licensed_window(case):
    w, worst = W.licence(case)
    a, ls, _, status = W.ref_case(case)
    print(f"self-check {case}: window={w} of {len(a.trace)} spread={worst:.3e} trials={[len(h['steps']) for h in ls.history[:w]]}")
    assert status in ("max_iter", "ok")
    assert w >= W.MIN_WINDOW, w
    assert worst <= W.LICENCE
    if case[0] == "lbfgs" and case[4] is None and all(h["task"] == "CONVERGENCE" for h in ls.history[:w]):
        assert a.updated[:w] == [1] * w and a.resets == 0  # the curvature condition: every pair of a free run is committed
    if case[4] is not None:  # the boxed form: no trial left the box, and some search was clipped by it
        lb, ub = W.box_of(case[2], case[4])
        assert all(np.all(h["x_k"] + t * h["d"] >= lb) and np.all(h["x_k"] + t * h["d"] <= ub) for h in ls.history[:w] for t, _, _ in h["steps"])
        assert any(h["stpmax"] < ls.t_max for h in ls.history[:w]) and ls.t_max == 1e10


def test_windows_cover_every_dcstep_case_and_a_stage_switch():
    seen, switches = set(), 0
    for case in ALL:
        for h in _searches(case):
            if len(h["steps"]) >= 2:
                seen.update(c for c in h["cases"] if c)
            switches += h["switched"]
    assert {1, 2, 3, 4} <= seen, seen
    assert switches >= 1


def _quartic(x):  # f = sum x^4 / 4 - x: minimum at 1
    return float(np.sum(0.25 * x ** 4 - x)), x ** 3 - 1.0


def test_iteration_cap_start_errors_and_the_non_finite_rule():
    x, d = np.array([0.0, 0.0]), np.array([4.0, 4.0])
    e = _quartic(x)
    o = R.CountingOracle(_quartic)
    assert RW.StrongWolfe().compute_step_len(x, e, d, o, 0) == 1.0 and o.calls == 0  # the first trial, unevaluated
    ls = RW.StrongWolfe()
    t1 = ls.compute_step_len(x, e, d, o, 1)
    assert o.calls == 1 and t1 != 1.0 and not ls.history[-1]["evaluated"] and ls.history[-1]["cases"] == [1]  # the NEXT step, unevaluated
    with pytest.raises(RW.NotDescent):
        RW.StrongWolfe().compute_step_len(x, e, -d, o, 5)
    with pytest.raises(RW.NotDescent):
        RW.StrongWolfe().compute_step_len(x, (e[0], np.zeros(2)), d, o, 5)
    # f = inf beyond a radius: the first trial (t = 1, |x| = 4 sqrt 2) is outside, the bracket [0, 1] is bisected until a trial is finite
    def walled(p):
        return (math.inf, np.full(2, math.nan)) if float(p @ p) > 4.0 else _quartic(p)
    ls = RW.StrongWolfe()
    t = ls.compute_step_len(x, e, d, R.CountingOracle(walled), 20)
    h = ls.history[-1]
    assert h["cases"][:2] == [5, 5] and [s[0] for s in h["steps"][:3]] == [1.0, 0.5, 0.25] and h["evaluated"] and h["task"] == "CONVERGENCE"
    assert math.isfinite(h["steps"][-1][1]) and float((x + t * d) @ (x + t * d)) <= 4.0
    # t_min: a trial at stpmin that fails the tests ends the search there
    ls = RW.StrongWolfe(t_min=1.0, t_max=1.0)
    assert ls.compute_step_len(x, e, d, R.CountingOracle(_quartic), 20) == 1.0 and ls.history[-1]["task"] == "WARNING: STP = STPMIN"


def test_boxed_form_stops_on_the_face_and_keeps_t_max():
    x, d = np.array([0.0, 0.0]), np.array([1.0, 0.5])
    lin = lambda p: (-float(p[0] + p[1]), np.array([-1.0, -1.0]))  # noqa: E731 -- unbounded below along d
    ls = RW.StrongWolfe(t_max=1e6, lower_bound=np.array([-1.0, -1.0]), upper_bound=np.array([3.0, 2.0]))
    t = ls.compute_step_len(x, lin(x), d, R.CountingOracle(lin), 20)
    assert t == 3.0 and ls.history[-1]["stpmax"] == 3.0 and ls.history[-1]["task"] == "WARNING: STP = STPMAX" and ls.t_max == 1e6
    assert [s[0] for s in ls.history[-1]["steps"]] == [1.0, 3.0]  # one trial away: the extrapolation is cut to the face
