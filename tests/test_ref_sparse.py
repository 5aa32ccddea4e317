"""CPU tests of tests/sparse_cases.py, and the self-checks that license every window tests/test_gpu_sparse.py compares on the GPU, by the method of
tests/test_ref_lbfgs.py: per case window = min(leading commits, above_f_floor, 30) (sparse_cases.SHORTER where that does not license), and inside
it the restatement's two-loop run, its compact-form run, its run with every dot product summed in reversed order and a run on the same function
with every ROW of Q summed in reversed order must take the same decisions and agree to 1e-11 in x and t -- a factor of 100 inside the 1e-9
max(1, ||x||) the GPU tests allow, because the GPU sums a row across lanes and f across workgroups, in a third order.  StrongWolfe is licensed
through tests/wolfe_cases.py's `agreement` (ls_cases among the decisions; math.fsum dot products among the runs).

Measured inside the windows (printed by every test below): free L-BFGS windows 14 to 29 with a spread of at most 8e-14, but ("bt", m = 1, arrow,
2050): 1.07e-11 at iteration 29, licensed to 28 (2.9e-12); SPG / projected gradient 29 at 1e-13; the boxes 5 and 7 (GLLQuadratic, cut in front of
the first iteration whose projected-gradient norm depends on the summation order) at 4e-16 at most; StrongWolfe 9 at n = 7, 14 and 30 with t_max = 0.5 at n = 2050, and an EMPTY window for the default settings at n = 2050
(sparse_cases.WOLFE_KNIFE_EDGE, explained there)."""
import numpy as np
import pytest

import lbfgs_cases as LC
import sparse_cases as SC
import wolfe_cases as W

LICENCE = SC.LICENCE


def test_csr_helper_equals_the_densified_product():
    rng = np.random.default_rng(11)
    for n in (7, 2050):
        for csr in (SC.tri(n), SC.arrow(n), SC.band(n, 20 if n > 7 else 3)):
            indptr, cols, vals = csr
            assert indptr[0] == 0 and indptr[-1] == cols.size == vals.size
            for i in range(n):
                assert np.all(np.diff(cols[indptr[i]:indptr[i + 1]]) > 0)
            q = SC.dense(csr)
            assert np.array_equal(q, q.T)
            x = rng.standard_normal(n)
            want = q @ x
            scale = np.abs(q) @ np.abs(x)
            for reverse in (False, True):
                assert np.all(np.abs(SC.matvec(csr, x, reverse) - want) <= 1e-14 * scale)
            f, g = SC.quadratic_fn(csr, SC.rhs(n))(x)
            assert np.all(np.abs(g - (want - SC.rhs(n))) <= 1e-14 * (scale + 1.0))
            assert abs(f - (0.5 * x @ want - SC.rhs(n) @ x)) <= 1e-12 * (1.0 + abs(f))


def test_matrices_are_what_the_module_says():
    n = 2050
    for name in SC.MATRICES:
        ev = np.linalg.eigvalsh(SC.dense(SC.matrix(name, n)))
        assert ev[0] > 0.0 and abs(ev[-1] / ev[0] - 101.0) < 1.0, (name, ev[0], ev[-1])
    q = SC.dense(SC.arrow(n))
    assert q[0, 0] == 3.04 and q[0, 1] == -1.0 and q[0, 9] == q[9, 0] == 0.5 / n * (1 + 9 % 7) / 7 and np.count_nonzero(q[0]) == n
    for h in (20, 350):
        b = SC.dense(SC.band(n, h))
        assert np.count_nonzero(b[n // 2]) == 2 * h + 1 and b[5, 7] == -1.0 / 3.0
        assert np.all(np.diag(b) - (np.abs(b).sum(axis=1) - np.diag(b)) > 0.039)
    x0 = SC.start(n)
    assert x0[0] == 0.5 and np.all(x0 >= 0.5) and np.all(x0 < 1.5)


def _spread(a, others, window):
    assert len(a.trace) >= window
    worst = 0.0
    for o in others:
        assert len(o.trace) >= window
        for k in range(window):
            assert a.trace[k]["n_evals"] == o.trace[k]["n_evals"] and a.trace[k]["ls_iters"] == o.trace[k]["ls_iters"], k
            assert getattr(a, "updated", [0] * window)[k] == getattr(o, "updated", [0] * window)[k], k
            # the norm of the projected gradient is compared on the GPU too (to 1e-7): it jumps when a coordinate sits one ulp off a bound in one run and on it in another
            assert abs(a.trace[k]["gnorm"] - o.trace[k]["gnorm"]) <= 1e-9 * max(1.0, a.trace[k]["gnorm"]), (k, a.trace[k]["gnorm"], o.trace[k]["gnorm"])
            worst = max(worst, float(np.linalg.norm(a.trace_x[k] - o.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k]))),
                        abs(a.trace[k]["t"] - o.trace[k]["t"]) / abs(a.trace[k]["t"]))
    return worst


def _self_check(case):
    a, _, _, _ = SC.ref_case(case)
    w = SC.window(case)
    worst = _spread(a, [r[0] for r in SC.other_runs(case)], w)
    print(f"self-check {case}: window={w} of {len(a.trace)} spread={worst:.3e}")
    assert worst <= LICENCE, worst
    return a, w


@pytest.mark.parametrize("case", SC.LBFGS_CASES + SC.FIRST_ORDER_CASES, ids=str)
def test_self_check_window(case):
    a, w = _self_check(case)
    assert w >= 14
    if case[0] == "lbfgs":
        assert w == min(LC.leading_commits(a), LC.above_f_floor(a, case[1]), SC.SHORTER.get(case, SC.WINDOW))
        if case[2] < 32:
            assert w > case[2]  # the ring wraps inside the window


@pytest.mark.parametrize("case", SC.BOX_CASES, ids=str)
def test_self_check_box(case):
    a, w = _self_check(case)
    assert w >= 5
    n, box = case[4], case[5]
    lb, ub = SC.box_of(n, box)
    assert all(r["t"] > 0.0 for r in a.trace[:w])
    x = a.trace_x[w - 1]
    assert np.all(x >= lb - SC.box_slack(box)) and np.all(x <= ub + SC.box_slack(box))
    active = int(np.sum((x == lb) | (x == ub)))
    assert 0 < active < n, active  # the box is active on some coordinates, not on all


@pytest.mark.parametrize("case", SC.WOLFE_CASES, ids=str)
def test_licensed_wolfe_window(case):
    w, worst = SC.wolfe_licence(case)
    a, ls, _, status = SC.ref_case(case)
    print(f"self-check {case}: window={w} of {len(a.trace)} spread={worst:.3e} trials={[len(h['steps']) for h in ls.history[:w]]}")
    assert status == "max_iter" and worst <= LICENCE
    if case in SC.WOLFE_KNIFE_EDGE:
        # iteration 0's stage bit alone separates the runs: the steps and iterates agree (module docstring of sparse_cases)
        others = SC.other_runs(case)
        diffs = {ls.history[0]["ls_cases"] ^ lo.history[0]["ls_cases"] for _, lo, _, _ in others}
        assert w == 0 and diffs == {0, 1 << 30}
        assert abs(ls.history[0]["steps"][-1][2]) < 1e-9 * abs(ls.history[0]["ginit"])  # phi' at the accepted trial: zero to rounding
        for b, _, _, _ in others:
            assert np.linalg.norm(a.trace_x[0] - b.trace_x[0]) <= LICENCE * np.linalg.norm(a.trace_x[0])
    else:
        assert w >= W.MIN_WINDOW
        assert sum(a.updated[:w]) == w  # the curvature condition keeps s.y > 0: every pair is committed


def test_self_check_big_n():
    a, _, _, status = SC.ref_big()
    assert status == "max_iter" and sum(a.updated) == SC.BIG_WINDOW > SC.BIG_M
    case = ("lbfgs", "bt", SC.BIG_M, "tri", SC.BIG_N, None)
    others = [SC.run_ref(case, iters=SC.BIG_WINDOW, dot=SC.rev_dot, direction="compact")[0], SC.run_ref(case, iters=SC.BIG_WINDOW, reverse=True)[0]]
    worst = _spread(a, others, SC.BIG_WINDOW)
    print(f"self-check n = 2^21 + 2: window={SC.BIG_WINDOW} spread={worst:.3e}")
    assert worst <= LICENCE, worst
    assert LC.above_f_floor(a, "bt") >= SC.BIG_WINDOW - 1
