"""CPU tests of the restatement tests/ref_cg.py, and the self-checks that license every window tests/test_gpu_cg.py compares on the GPU (the method
of tests/test_ref_lbfgs.py): each case runs with numpy.dot, with math.fsum of the products and with every dot product summed in reversed order,
and the window (cg_cases.licence) ends at the first iteration where the iterates differ by more than 1e-11 max(1, ||x||) (or t by 1e-11 |t|),
n_evals differs, the restart pattern differs, or f's decrease falls below lbfgs_cases.above_f_floor's 1e4 ulp.  That is a factor of 100 inside
the 1e-9 max(1, ||x||) the GPU tests allow, because the GPU sums in a fourth order, across workgroups.

The device-objective cases ("lse", "quad") also run with every evaluation moved by a few ulp (cg_cases.rounded_otherwise: the device evaluates the
same function with other roundings) and their windows end where that moves x, t or beta by more than 2.5e-10.

Windows measured (printed by test_self_check_window): 8 (dy, log-sum-exp, n = 7, StrongWolfe) to 29 of 30; the worst disagreement between summation
orders inside a window is 9.2e-12 (log-sum-exp, n = 2050); the separable quartic and the quadratic at n = 2050 stay below 1e-13.  Restarts inside the windows: Powell's test in most BackTracking cases (its steps leave g+.g large), truncations of PR+ and
HS+ to 0 on the quartic and the quadratic under BackTracking, scheduled restarts in cg_cases.EVERY."""
import math

import numpy as np
import pytest

import cg_cases as C
import ref_cg as RC


@pytest.mark.parametrize("variant,oracle,ls,n", C.CASES)
def test_self_check_window(variant, oracle, ls, n):
    w, worst = C.licence(variant, oracle, ls, n)
    a = C.ref_case(variant, oracle, ls, n)[0]
    print(f"self-check {(variant, oracle, ls, n)}: window={w} of {len(a.trace)} spread={worst:.3e} restarts={a.why[:w]}")
    assert w >= C.MIN_WINDOW, w
    assert worst <= C.LICENCE, worst


def test_case_set_covers_every_rule_inside_licensed_windows():
    seen = {}
    for c in C.CASES:
        w = C.window(*c)
        a = C.ref_case(*c)[0]
        for why in a.why[:w]:
            if why:
                seen.setdefault(why, set()).add(c[0])
    assert {c[0] for c in C.CASES} == set(RC.VARIANTS)
    assert seen.get("powell")
    assert seen.get("truncated") and seen["truncated"] <= {"pr+", "hs+"}
    v, o, ls, n, nu, every = C.EVERY
    w, worst = C.licence(v, o, ls, n, nu, every)
    a = C.ref_case(v, o, ls, n, "numpy", nu, every)[0]
    assert w >= C.MIN_WINDOW and worst <= C.LICENCE
    assert a.why[:w].count("every") >= 2 and a.updated[:w] == [0 if k % 3 == 2 else 1 for k in range(w)]
    # Powell's test on and off: the default run restarts by it inside its window, nu = inf never does
    on = C.ref_case(*C.POWELL)[0]
    off = C.ref_case(*C.POWELL, "numpy", float("inf"))[0]
    w_off, worst_off = C.licence(*C.POWELL, float("inf"))
    assert "powell" in on.why[:C.window(*C.POWELL)] and "powell" not in off.why
    assert w_off >= C.MIN_WINDOW and worst_off <= C.LICENCE


def test_formulas_by_hand():
    sums = dict(gpgp=4.0, gpy=3.0, dy=2.0, gpd=0.5, yy=5.0, dd=9.0, gg=8.0)
    assert RC.beta_formula("fr", **sums) == 0.5
    assert RC.beta_formula("pr+", **sums) == 0.375
    assert RC.beta_formula("hs+", **sums) == 1.5
    assert RC.beta_formula("dy", **sums) == 2.0
    beta_n = (3.0 - (10.0 * 0.5) / 2.0) / 2.0
    eta = -1.0 / (3.0 * 0.01)
    assert RC.beta_formula("hz", **sums) == beta_n == 0.25 and eta < beta_n
    neg = dict(sums, gpy=-3.0)
    assert RC.beta_formula("pr+", **neg) == 0.0 and RC.beta_formula("hs+", **neg) == 0.0
    assert RC.beta_formula("hz", **dict(sums, gpy=-1e9)) == eta  # the lower bound eta_k
    zero = dict(sums, dy=0.0, gg=0.0)
    assert math.isinf(RC.beta_formula("fr", **zero)) and math.isinf(RC.beta_formula("dy", **zero))
    assert math.isnan(RC.beta_formula("fr", **dict(zero, gpgp=0.0)))
    assert RC.beta_formula("pr+", **dict(zero, gpy=0.0)) == 0.0  # NaN > 0 is false


def test_rules_on_a_constant_gradient():
    """y = 0: every denominator with y vanishes.  FR's beta is 1 and Powell's test (|g+.g| = g+.g+) zeroes it; with nu = inf FR keeps beta = 1;
    DY's 1 / 0 is not finite (rule 4)"""
    c = np.array([1.0, -2.0, 0.5])
    fn = lambda x: (float(c @ x), c.copy())  # noqa: E731
    s, _, _ = C.run_ref(fn, np.zeros(3), "fr", "bt", 3)
    assert s.updated == [0, 0, 0] and s.why == ["powell"] * 3 and s.restarts == 3
    s, _, _ = C.run_ref(fn, np.zeros(3), "fr", "bt", 3, powell_nu=float("inf"))
    assert s.updated == [1, 1, 1] and s.betas == [1.0, 1.0, 1.0] and s.restarts == 0
    assert np.array_equal(s.directions[2], 1.0 * (1.0 * -c - c) - c)
    s, _, _ = C.run_ref(fn, np.zeros(3), "dy", "bt", 3, powell_nu=float("inf"))
    assert s.why == ["not finite"] * 3 and all(np.array_equal(d, -c) for d in s.directions)


def test_first_direction_is_minus_g_and_drop_p():
    fn, x0 = C.oracle_fn("host", 7)
    s, _, _ = C.run_ref(fn, x0, "pr+", "wolfe", 4)
    assert np.array_equal(s.directions[0], -fn(x0)[1]) and s.updated[0] == 1 and s.restarts == 0
    assert not np.array_equal(s.directions[1], -fn(s.trace_x[0])[1])
    x = s.x.copy()
    s.drop_p()
    C.run_ref(fn, None, "pr+", "wolfe", 1, solver=s)
    assert np.array_equal(s.directions[4], -fn(x)[1]) and s.restarts == 0


@pytest.mark.parametrize("variant", RC.VARIANTS)
def test_two_calls_are_one(variant):
    fn, x0 = C.oracle_fn("host", 7)
    one, _, _ = C.run_ref(fn, x0, variant, "wolfe", 8)
    two, _, _ = C.run_ref(fn, x0, variant, "wolfe", 4)
    C.run_ref(fn, None, variant, "wolfe", 4, solver=two)
    assert np.array_equal(one.x, two.x) and one.betas == two.betas and one.restarts == two.restarts


@pytest.mark.parametrize("n", C.SHAPE_SIZES)
def test_beta_bound_holds_for_three_summation_orders(n):
    """the derivation of cg_cases.beta_bound against float64 itself: beta of the second iteration from sums in numpy's, the reversed and (up to
    n = 4099) fsum's order lies within the bound of the longdouble value, for every variant"""
    fn, x0 = C.oracle_fn("host", n)
    for variant in RC.VARIANTS:
        s, _, _ = C.run_ref(fn, x0, variant, "wolfe", 2, powell_nu=float("inf"))
        g, gp, d = fn(s.trace_x[0])[1], fn(s.trace_x[1])[1], s.directions[1]
        exact, mags = C.ld_sums(g, gp, d)
        centre, bound = C.beta_bound(variant, n, exact, mags)
        y = gp - g
        for name, dot in C.DOTS.items():
            if name == "fsum" and n > 4099:
                continue
            sums = dict(gpgp=float(dot(gp, gp)), gpy=float(dot(gp, y)), dy=float(dot(d, y)), gpd=float(dot(gp, d)), yy=float(dot(y, y)),
                        dd=float(dot(d, d)), gg=float(dot(g, g)))
            b = RC.beta_formula(variant, **sums)
            assert abs(b - centre) <= bound, (variant, name, b, centre, bound)
        assert s.betas[1] != 0.0 and abs(s.betas[1] - centre) <= bound
        print(f"n={n} {variant}: beta={centre:.6e} bound={bound:.3e} ({bound / abs(centre):.1e} relative)")
