"""CPU tests of tests/ref_broyden.py, the restatement the GPU solver QN_BROYDEN is compared with (tests/test_gpu_broyden.py): it reproduces the
assertions of the reference's own tests, and every window of tests/broyden_cases.py is licensed -- finite, a real update at every step, a
clearly non-symmetric H at its end, and an order spread (four floating-point orders of the same statements) below the cap the cases file
states.  The measured spreads are printed (-s) and recorded in tests/broyden_cases.py, where the GPU tolerances come from."""
import numpy as np
import pytest

import broyden_cases as BC
import ref_broyden as R


@pytest.mark.parametrize("name,ls,bounded", BC.REFERENCE_TESTS)
def test_reference_tests_assertions(name, ls, bounded):
    """broyden.rs:135-234, broyden_b.rs:166-222: minimize(..., 1000, 100000).unwrap(); assert f < 1e-6; has_converged"""
    pr = dict(fn=BC.two_var(1.0), x0=BC.X0_2D.copy(), lb=-BC.INF2 if bounded else None, ub=BC.INF2 if bounded else None)
    s, o, status = BC.run_ref(pr, ls, 1000, max_ls=100000)
    assert status == "ok"
    f, g = pr["fn"](s.x)
    assert abs(f - 0.0) < 1e-6
    assert s.has_converged((f, g))


def test_update_is_the_written_one_not_the_textbook_one():
    """H+ = H + ((s - H y) s') H / (s . y): w = H' s (not H s), denominator s.y (not s'Hy) -- the secant equation does not hold"""
    rng = np.random.default_rng(1)
    n = 6
    h = np.eye(n) + 0.3 * rng.standard_normal((n, n))
    s, y = rng.standard_normal(n), rng.standard_normal(n)
    lit, fac = R.broyden_update(h, s, y, "literal"), R.broyden_update(h, s, y, "factored")
    assert BC.rel_diff(fac, lit) < 1e-14
    a = s - h @ y
    assert BC.rel_diff(h + np.outer(a, h.T @ s) / (s @ y), lit) < 1e-14
    assert BC.rel_diff(h + np.outer(a, h @ s) / (s @ y), lit) > 1e-2   # w = H s is another matrix
    assert np.max(np.abs(lit @ y - s)) > 1e-2                            # H+ y != s


@pytest.mark.parametrize("name", list(BC.WINDOWS))
def test_window_is_licensed(qo, name):
    w = BC.WINDOWS[name]
    pr = BC.problem(w, qo)
    s, o, status = BC.run_ref(pr, w["ls"], w["K"])
    assert status == "max_iter" and s.k == w["K"]
    assert all(r["updated"] == 1 for r in s.trace)
    assert np.all(np.isfinite(s.h)) and np.all(np.isfinite(np.array(s.trace_x))) and all(np.isfinite(r["f"]) for r in s.trace)
    asym = float(np.max(np.abs(s.h - s.h.T)))
    assert asym > 1e-6 * float(np.max(np.abs(s.h))), asym
    if pr["lb"] is not None:
        assert np.all(np.array(s.trace_x) >= pr["lb"]) and np.all(np.array(s.trace_x) <= pr["ub"])
    spread = BC.spread_of(pr, w)
    print(f"{name}: K = {w['K']}  order spread = {spread:.3e}  recorded = {w['spread']:.3e}  GPU tolerance = {BC.tolerance(w):.3e}  asym = {asym:.3e}")
    assert spread < BC.SPREAD_CAP
    assert w["spread"] < BC.SPREAD_CAP and BC.tolerance(w) <= BC.MARGIN * BC.SPREAD_CAP


def test_skip_case_reaches_the_skip_rule(qo):
    w = BC.SKIP_CASE
    s, o, status = BC.run_ref(BC.problem(w, qo), w["ls"], w["K"])
    assert status == "ok" and s.k < w["K"]
    assert s.trace[-1]["updated"] == 0 and s.s_norm < BC.TOL and s.next_iterate_too_close()
