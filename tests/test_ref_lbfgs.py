"""CPU tests of the restatement tests/ref_lbfgs.py, and the self-checks that license every window tests/test_gpu_lbfgs.py compares on the GPU
(the method of tests/test_ref_pnewton.py): on each case the two-loop recursion, the compact form and the two-loop recursion with every dot
product summed in reversed order must give the same decisions and iterates that agree to 1e-11 -- a factor of 100 inside the 1e-9 max(1, ||x||) the
GPU tests allow, because the GPU sums in a third order, across workgroups.  Windows: lbfgs_cases.window / box_window (at most 30 iterations,
kappa = 1e2, tol 1e-10).

Worst relative divergence (in x, and in the step t) measured inside the chosen windows (printed by every test below): 9.2e-12 (lse,
GLLQuadratic, m = 1, n = 2050; the other log-sum-exp cases at n = 2050 up to 6.6e-12); the box cases stay below 2.1e-14, n = 2^21 + 2 at 4.7e-16, the
unit-scaling window at 2.3e-15; unit-scaled L-BFGS against tests/ref_python.py's dense BFGS: 4.6e-15."""
import numpy as np
import pytest

import lbfgs_cases as C
import ref_lbfgs as RL
import ref_python as RP
import ref_spg as R
import spg_cases as S

LICENCE = 1e-11  # x 100 < 1e-9


def rev_dot(a, b):
    return float(np.dot(a[::-1], b[::-1]))


def _spread(a, others, window):
    assert len(a.trace) >= window
    worst = 0.0
    for o in others:
        assert len(o.trace) >= window
        for k in range(window):
            assert a.trace[k]["n_evals"] == o.trace[k]["n_evals"] and a.trace[k]["ls_iters"] == o.trace[k]["ls_iters"], k
            assert a.updated[k] == o.updated[k], k
            worst = max(worst, float(np.linalg.norm(a.trace_x[k] - o.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k]))),
                        abs(a.trace[k]["t"] - o.trace[k]["t"]) / abs(a.trace[k]["t"]))
    return worst


def _self_check(name, a, fn, x0, lb, ub, ls, m, iters, window, unit=False, runs=("compact", "reversed")):
    others = []
    if "compact" in runs:
        others.append(C.run_ref(fn, x0, lb, ub, ls, m, iters, unit=unit, direction="compact")[0])
    if "reversed" in runs:
        others.append(C.run_ref(fn, x0, lb, ub, ls, m, iters, unit=unit, dot=rev_dot)[0])
    if "compact_reversed" in runs:
        others.append(C.run_ref(fn, x0, lb, ub, ls, m, iters, unit=unit, dot=rev_dot, direction="compact")[0])
    worst = _spread(a, others, window)
    print(f"self-check {name}: window={window} of {len(a.trace)} spread={worst:.3e}")
    assert worst <= LICENCE, worst
    return worst


def test_two_loop_equals_compact_form_on_random_pairs():
    rng = np.random.default_rng(0)
    for n, k in ((3, 1), (7, 5), (40, 12)):
        a = rng.standard_normal((n, n))
        h = a @ a.T + n * np.eye(n)
        pairs = []
        for _ in range(k):
            s = rng.standard_normal(n)
            pairs.append((s, h @ s))
        g = rng.standard_normal(n)
        for gamma in (1.0, 0.37):
            assert np.allclose(RL.two_loop(pairs, g, gamma, np.dot), RL.compact(pairs, g, gamma, np.dot), rtol=1e-9, atol=1e-12)
    # n pairs from an SPD quadratic with gamma = 1 span everything: H_k = H^-1 exactly (BFGS on a quadratic, conjugate pairs aside: use the secant property)
    s, y = pairs[-1]
    assert np.allclose(RL.two_loop(pairs, y, 0.37, np.dot), s, rtol=1e-9)  # H_k y_k = s_k


@pytest.mark.parametrize("oracle,ls,m,n", [c for c in C.CASES if c[0] != "quad"])  # ("quad" is "host"'s function on the device)
def test_self_check_window(oracle, ls, m, n):
    fn, x0 = C.oracle_fn(oracle, n)
    lb, ub = C.free_box(n)
    a, _, _ = C.ref_case(oracle, ls, m, n)
    w = C.window(oracle, ls, m, n)
    assert w >= min(4, len(a.trace))  # (n = 2 is at rounding level after 4 .. 6 iterations)
    if m < 32 and n > 2:
        assert w > m  # the ring wraps inside the window
    _self_check((oracle, ls, m, n), a, fn, x0, lb, ub, ls, m, C.WINDOW, w)
    if oracle == "host":
        assert C.window("quad", ls, m, n) == w


@pytest.mark.parametrize("ls,n,m", C.BOX_CASES)
def test_self_check_box(ls, n, m):
    fn, x0 = C.oracle_fn("quad", n)
    lb, ub = S.bounds(n, C.BOX)
    a, _, _ = C.ref_box_case(ls, n, m)
    w = C.box_window(ls, n, m)
    _self_check(("box", ls, n, m), a, fn, x0, lb, ub, ls, m, C.WINDOW, w)
    if m < 5 or ls == "gll":
        assert sum(a.updated[:w]) > m  # the ring wraps with the box active
    x = a.trace_x[w - 1]
    active = int(np.sum((x == lb) | (x == ub)))
    assert 0 < active < n, active  # the box is active on some coordinates, not on all


def test_self_check_big_n():
    fn, x0 = C.separable_problem()
    lb, ub = C.free_box(C.BIG_N)
    a, _, status = C.ref_big()
    assert status == "max_iter" and sum(a.updated) == C.BIG_WINDOW > C.BIG_M
    _self_check("n = 2^21 + 2", a, fn, x0, lb, ub, "bt", C.BIG_M, C.BIG_WINDOW, C.BIG_WINDOW, runs=("compact_reversed",))


def test_unit_scaling_is_dense_bfgs_while_nothing_is_dropped():
    """gamma = 1 and k <= m: the L-BFGS matrix IS the BFGS matrix built from H = I -- against tests/ref_python.py's dense BFGS + BackTracking"""
    worst = 0.0
    for n, m, iters in ((8, 12, 12), (C.UNIT_N, C.UNIT_M, C.UNIT_WINDOW)):
        if n == C.UNIT_N:
            fn, x0 = C.unit_problem()
        else:
            fn, x0 = C.oracle_fn("host", 7)[0], None
            q, b, x0, _ = C.quad_problem(n)
            fn = R.quadratic_fn(q, b)
        lb, ub = C.free_box(n)
        a, _, _ = C.run_ref(fn, x0, lb, ub, "bt", m, iters, unit=True)
        assert len(a.trace) == iters and sum(a.updated) == iters <= m
        if n == C.UNIT_N:
            _self_check("unit scaling", a, fn, x0, lb, ub, "bt", m, iters, iters, unit=True)
        for upto in ((iters,) if n == C.UNIT_N else range(1, iters + 1)):
            status, x, k, _, _, steps = RP.minimize("bfgs", C.TOL, list(x0), RP.BackTracking(1e-4, 0.5), lambda p: fn(np.array(p)), upto, 50)
            assert status == "max_iter" and k == upto
            assert steps == [r["t"] for r in a.trace[:upto]]
            worst = max(worst, float(np.linalg.norm(np.array(x) - a.trace_x[upto - 1]) / max(1.0, np.linalg.norm(x))))
    print(f"unit-scaled L-BFGS against dense BFGS: spread={worst:.3e}")
    assert worst <= LICENCE, worst


def test_commit_rule_and_safeguard_by_hand():
    inf2 = np.array([np.inf, np.inf])
    # a constant gradient: y = 0, the pair is never committed
    c = np.array([1.0, -2.0])
    s, _, _ = C.run_ref(lambda x: (float(c @ x), c.copy()), np.zeros(2), -inf2, inf2, "bt", 5, 3)
    assert s.updated == [0, 0, 0] and s.stored_pairs() == 0 and s.resets == 0
    # a concave slice: s.y < 0 is not committed either -- every stored pair has s.y > 0, so H_k is positive definite in exact arithmetic and
    # g.z <= 0 can only come from rounding, overflow or g = 0.  Here two pairs are stored first, then the steps run along the concave coordinate.
    s, _, _ = C.run_ref(C.concave_mixed_fn, np.array(C.CONCAVE_X0), -inf2, inf2, "bt", 5, C.CONCAVE_WINDOW)
    assert s.updated == [1, 1, 0, 0, 0] and s.stored == [1, 2, 2, 2, 2] and s.resets == 0
    assert len(s.pairs) == 2 and all(float(a @ b) > 0.0 for a, b in s.pairs)
    # g = 0 exactly with tol = 0: g.z = 0 is not > 0 -- the memory is cleared and counted
    s, _, _ = C.run_ref(lambda x: (0.5 * float(x @ x), x.copy()), np.array([3.0, 4.0]), -inf2, inf2, "bt", 5, 3, tol=0.0)
    assert s.updated == [1, 0, 0] and s.resets == 1 and s.stored_pairs() == 0 and np.array_equal(s.x, [0.0, 0.0])


@pytest.mark.parametrize("m", C.REJECT_MEMORIES)
def test_self_check_rejected_pair_with_pairs_in_the_memory(m):
    """lbfgs_cases.reject_fn: the second and third steps lie in the linear band (y = 0) with one pair stored -- a FULL memory at m = 1 -- and the
    run goes on storing pairs afterwards"""
    a, _, _ = C.ref_reject(m)
    w = C.reject_window(m)
    assert a.updated[:4] == [1, 0, 0, 1] and a.stored[:4] == [1, 1, 1, min(m, 2)] and w >= 5 and a.resets == 0
    lb, ub = C.free_box(len(C.REJECT_X0))
    _self_check(("reject", m), a, C.reject_fn, np.array(C.REJECT_X0), lb, ub, "bt", m, C.REJECT_WINDOW, w)
    b, _, _ = C.run_ref(C.concave_mixed_fn, np.array(C.CONCAVE_X0), *C.free_box(2), "bt", m, C.CONCAVE_WINDOW)
    _self_check(("concave", m), b, C.concave_mixed_fn, np.array(C.CONCAVE_X0), *C.free_box(2), "bt", m, C.CONCAVE_WINDOW, C.CONCAVE_WINDOW)
