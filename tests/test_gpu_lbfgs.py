"""GPU tests of limited-memory BFGS (QN_LBFGS: LBFGS / ProjectedLBFGS; kernels csrc/qn_lbfgs.hip.h) against the restatement tests/ref_lbfgs.py,
whose direction is the two-loop recursion where the GPU runs the compact form.  Windows and the tolerance (1e-9 max(1, ||x||), the family's)
are licensed case by case by tests/test_ref_lbfgs.py.  Every direction on its own, through whole runs with a full and wrapping memory: tests/test_gpu_lbfgs_replay.py.

The safeguard case.  Every stored pair has s.y > DBL_EPSILON y.y > 0, so H_k is positive definite in exact arithmetic: a concave slice cannot
make g.z <= 0 -- its pair is simply not stored (checked below: no reset, the iterates follow the restatement).  g.z <= 0 needs rounding,
overflow or g = 0; the case that asserts resets() >= 1 reaches g = 0 exactly with tol = 0."""
import os
import subprocess

import numpy as np
import pytest

import lbfgs_cases as C
import ref_spg as R
import spg_cases as S
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH_VECTOR, PATH_PNEWTON, PATH_LBFGS = 64, 128, 1024


def _ls(qn, kind, lb, ub):
    if kind == "gll":
        return qn.GLLQuadratic(1e-4, 10)
    if kind == "bt":
        return qn.BackTracking(1e-4, 0.5)
    return qn.BackTrackingB(1e-4, 0.5, lb, ub)


def _gpu(qn, oracle, x0, lb, ub, ls, m, iters, memoize=None, tol=C.TOL, unit=False, max_ls=50):
    s = qn.ProjectedLBFGS(tol, x0, lb, ub, m=m, memoize=memoize)
    if unit:
        s.set_option("lbfgs_unit_scaling", 1)
    s.set_trace(iters, with_x=True)
    status = "ok"
    try:
        s.minimize(_ls(qn, ls, lb, ub), oracle, iters, max_ls)
    except qn.MaxIterReached:
        status = "max_iter"
    return s, status


def _device_oracle(qn, oracle, n):
    if oracle == "lse":
        a, c, mu, _, _, _ = C.lse_problem(n)
        return qn.LogSumExp(a, c, mu)
    q, b, _, _ = C.quad_problem(n)
    return qn.Quadratic(q, b) if oracle == "quad" else R.quadratic_fn(q, b)


def _compare_updates(s, ref, window, fn, x0):
    """`updated`, s_norm and f of the trace against the restatement.  The bound on f: the iterates are licensed to 1e-9 max(1, ||x||), so
    f(x_k) may move by ||g(x_k)||_2 times that (first order; the windows end long before second order matters); on top, a device objective sums
    f in another order than numpy -- at most 2^21 terms, blocked sums: ~sqrt(n) eps = 3e-13 of the sum of magnitudes, which at kappa = 1e2 stays
    within ~30 |f| -- 1e-11 max(1, |f|)."""
    tr, _ = s.trace()
    assert [r["updated"] for r in tr[:window]] == ref.updated[:window]
    for k in range(window):
        assert abs(tr[k]["s_norm"] - ref.trace[k]["s_norm"]) <= 1e-9 * max(1.0, ref.trace[k]["s_norm"]), k
        xk = ref.trace_x[k - 1] if k else R.box_projection(np.asarray(x0, dtype=np.float64), ref.lb, ref.ub)
        fr = ref.trace[k]["f"]
        bound = 1e-9 * max(1.0, float(np.linalg.norm(xk))) * float(np.linalg.norm(fn(xk)[1])) + 1e-11 * max(1.0, abs(fr))
        assert abs(tr[k]["f"] - fr) <= bound, (k, tr[k]["f"], fr, bound)


@pytest.mark.parametrize("oracle,ls,m,n", C.CASES)
def test_parity_window(qn, oracle, ls, m, n):
    ref, _, _ = C.ref_case(oracle, ls, m, n)
    w = C.window(oracle, ls, m, n)
    fn, x0 = C.oracle_fn(oracle, n)
    lb, ub = C.free_box(n)
    s, status = _gpu(qn, _device_oracle(qn, oracle, n), x0, lb, ub, ls, m, w)
    assert status == "max_iter"
    ref_w = type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
    _compare(s, ref_w, w)
    _compare_updates(s, ref, w, fn, x0)
    assert s.memory == m and s.stored_pairs() == min(m, sum(ref.updated[:w]))
    assert s.stats()["path"] & PATH_LBFGS and s.stats()["path"] & PATH_VECTOR and not s.stats()["path"] & PATH_PNEWTON


def test_parity_grid_stride_wraps(qn):
    """n = 2^21 + 2: more than 1024 workgroups' worth of elements; m = 3, a separable function on a host closure"""
    ref, _, _ = C.ref_big()
    fn, x0 = C.separable_problem()
    lb, ub = C.free_box(C.BIG_N)
    s, status = _gpu(qn, fn, x0, lb, ub, "bt", C.BIG_M, C.BIG_WINDOW)
    assert status == "max_iter"
    _compare(s, ref, C.BIG_WINDOW)
    _compare_updates(s, ref, C.BIG_WINDOW, fn, x0)
    assert s.stored_pairs() == C.BIG_M


@pytest.mark.parametrize("ls,n,m", C.BOX_CASES)
def test_projected_parity_window(qn, ls, n, m):
    ref, _, _ = C.ref_box_case(ls, n, m)
    w = C.box_window(ls, n, m)
    q, b, x0, _ = C.quad_problem(n)
    lb, ub = S.bounds(n, C.BOX)
    s, status = _gpu(qn, qn.Quadratic(q, b), x0, lb, ub, ls, m, w)
    assert status == "max_iter"
    ref_w = type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
    _compare(s, ref_w, w)
    _compare_updates(s, ref, w, R.quadratic_fn(q, b), x0)
    assert s.stored_pairs() == ref.stored[w - 1]
    x = s.x()
    assert np.all(x >= lb) and np.all(x <= ub) and 0 < int(np.sum((x == lb) | (x == ub))) < n


def test_unit_scaling_equals_dense_bfgs(qn):
    fn, x0 = C.unit_problem()
    n, w = C.UNIT_N, C.UNIT_WINDOW
    q, b, _, _ = C.quad_problem(n)
    lb, ub = C.free_box(n)
    obj = qn.Quadratic(q, b)
    s = qn.LBFGS(C.TOL, x0, m=C.UNIT_M)
    s.set_option("lbfgs_unit_scaling", 1)
    s.set_trace(w, with_x=True)
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.BackTracking(1e-4, 0.5), obj, w, 50)
    d = qn.BFGS(C.TOL, x0)
    d.set_trace(w, with_x=True)
    with pytest.raises(qn.MaxIterReached):
        d.minimize(qn.BackTracking(1e-4, 0.5), obj, w, 50)
    (ta, xa), (tb, xb) = s.trace(), d.trace()
    assert len(ta) == len(tb) == w and s.gamma() == 1.0 and s.stored_pairs() == w
    for k in range(w):
        assert abs(ta[k]["t"] - tb[k]["t"]) <= 1e-9 * abs(tb[k]["t"]), k
        assert np.linalg.norm(xa[k] - xb[k]) <= 1e-9 * max(1.0, np.linalg.norm(xb[k])), k
    ref, _, _ = C.run_ref(fn, x0, lb, ub, "bt", C.UNIT_M, w, unit=True)
    _compare(s, ref, w)
    _compare_updates(s, ref, w, fn, x0)


def test_commit_rule_constant_gradient(qn):
    c = np.array([1.0, -2.0, 0.5])
    fn = lambda x: (float(c @ x), c.copy())  # noqa: E731
    lb, ub = C.free_box(3)
    ref, _, _ = C.run_ref(fn, np.zeros(3), lb, ub, "bt", 5, 3)
    s, _ = _gpu(qn, fn, np.zeros(3), lb, ub, "bt", 5, 3)
    _compare(s, ref, 3)
    tr, _ = s.trace()
    assert [r["updated"] for r in tr] == [0, 0, 0] == ref.updated and s.stored_pairs() == 0 and s.resets() == 0


@pytest.mark.parametrize("m", C.REJECT_MEMORIES)
def test_rejected_pair_leaves_a_non_empty_memory_as_it_was(qn, m):
    """lbfgs_cases.reject_fn: one pair is stored, the next two steps have y = 0 exactly and are rejected -- with a FULL memory at m = 1, with one
    pair of m at m = 2, 5 -- and the run goes on storing pairs (at m = 1 into the slot the rejected pairs were staged in, dropping the old one).
    A staging write into a live slot, or a head / count / Gram row mishandled after a rejection, changes the iterates that follow."""
    ref, _, _ = C.ref_reject(m)
    w = C.reject_window(m)
    x0 = np.array(C.REJECT_X0)
    lb, ub = C.free_box(x0.size)
    s = qn.LBFGS(C.TOL, x0, m=m)
    s.set_trace(w, with_x=True)
    stored = []
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.BackTracking(1e-4, 0.5), C.reject_fn, w, 50, callback=lambda r: stored.append(r.stored_pairs()))
    ref_w = type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
    _compare(s, ref_w, w)
    _compare_updates(s, ref, w, C.reject_fn, x0)
    assert ref.updated[:4] == [1, 0, 0, 1] and w >= 5  # at least one stored pair behind the rejected ones is compared
    assert stored == ref.stored[:w] and stored[:3] == [1, 1, 1]
    assert s.resets() == 0


def test_rejected_pair_concave_step_memoized(qn):
    """the same bookkeeping through the memoised path (memoize = 1: the accepted trial's evaluation is the update's): concave_mixed_fn, m = 2, so
    the two stored pairs FILL the memory before the rejections"""
    fn, x0, w = C.concave_mixed_fn, np.array(C.CONCAVE_X0), C.CONCAVE_WINDOW
    lb, ub = C.free_box(2)
    ref, _, _ = C.run_ref(fn, x0, lb, ub, "bt", 2, w)
    s = qn.LBFGS(C.TOL, x0, m=2, memoize=1)
    s.set_trace(w, with_x=True)
    stored = []
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.BackTracking(1e-4, 0.5), fn, w, 50, callback=lambda r: stored.append(r.stored_pairs()))
    tr, xs = s.trace()
    assert [r["updated"] for r in tr] == ref.updated == [1, 1, 0, 0, 0] and stored == ref.stored == [1, 2, 2, 2, 2]
    for k in range(w):
        assert np.linalg.norm(xs[k] - ref.trace_x[k]) <= 1e-9 * max(1.0, np.linalg.norm(ref.trace_x[k])), k
        assert abs(tr[k]["t"] - ref.trace[k]["t"]) <= 1e-9 * abs(ref.trace[k]["t"]), k


def test_safeguard(qn):
    lb, ub = C.free_box(2)
    # a concave slice: two pairs are stored on the convex coordinate, then the pairs with s.y < 0 are not; nothing is reset (module docstring)
    fn, x0, w = C.concave_mixed_fn, np.array(C.CONCAVE_X0), C.CONCAVE_WINDOW
    ref, _, _ = C.run_ref(fn, x0, lb, ub, "bt", 5, w)
    s, _ = _gpu(qn, fn, x0, lb, ub, "bt", 5, w)
    _compare(s, ref, w)
    _compare_updates(s, ref, w, fn, x0)
    assert ref.updated == [1, 1, 0, 0, 0]
    assert s.resets() == ref.resets == 0 and s.stored_pairs() == ref.stored_pairs() == 2
    # g = 0 exactly, tol = 0: g.z = 0 is not > 0 -- the memory is cleared, z = g, the iterates follow the restatement
    fn = lambda x: (0.5 * float(x @ x), x.copy())  # noqa: E731
    ref, _, _ = C.run_ref(fn, np.array([3.0, 4.0]), lb, ub, "bt", 5, 3, tol=0.0)
    s, _ = _gpu(qn, fn, np.array([3.0, 4.0]), lb, ub, "bt", 5, 3, tol=0.0)
    _compare(s, ref, 3)
    _compare_updates(s, ref, 3, fn, np.array([3.0, 4.0]))
    assert s.resets() >= 1 and s.resets() == ref.resets and s.stored_pairs() == 0 and s.gamma() == 1.0


def test_determinism(qn):
    n = 2050
    q, b, x0, _ = C.quad_problem(n)
    lb, ub = S.bounds(n, C.BOX)
    obj = qn.Quadratic(q, b)
    runs = [_gpu(qn, obj, x0, lb, ub, "gll", 5, 30)[0].trace()[1].copy() for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()


@pytest.mark.parametrize("oracle", ["host", "lse"])
def test_memoize_and_counts(qn, oracle):
    n, ls, m = 7, "gll", 5
    ref, o, _ = C.ref_case(oracle, ls, m, n)
    w = C.window(oracle, ls, m, n)
    ref_w, o_w, _ = C.run_ref(*C.oracle_fn(oracle, n), *C.free_box(n), ls, m, w)
    _, x0 = C.oracle_fn(oracle, n)
    lb, ub = C.free_box(n)
    xs, evals = [], []
    for memo in (0, 1):
        calls = []
        dev = _device_oracle(qn, oracle, n)
        if oracle == "host":
            inner = dev

            def dev(x, inner=inner, calls=calls):
                calls.append(1)
                return inner(x)
        s, _ = _gpu(qn, dev, x0, lb, ub, ls, m, w, memoize=memo)
        xs.append(s.trace()[1].copy())
        st = s.stats()
        assert st["oracle_calls"] == o_w.calls  # the restatement's call sequence, whatever is memoised
        evals.append(st["oracle_evals"])
        if oracle == "host":
            assert len(calls) == st["oracle_evals"]
    assert xs[0].tobytes() == xs[1].tobytes()
    assert evals[0] == o_w.calls and evals[1] < evals[0]
    # memoised: the loop top's and the update's evaluations are the line search's last trial -- one evaluation per trial, one for x0
    assert evals[1] == 1 + sum(r["ls_iters"] for r in ref_w.trace[:w])


def test_warm_restart_reset_and_rejections(qn):
    n = 2050
    q, b, x0, _ = C.quad_problem(n)
    lb, ub = C.free_box(n)
    obj = qn.Quadratic(q, b)
    one, _ = _gpu(qn, obj, x0, lb, ub, "gll", 5, 20)
    two = qn.LBFGS(C.TOL, x0, m=5)
    ls = qn.GLLQuadratic(1e-4, 10)
    for _ in range(2):
        with pytest.raises(qn.MaxIterReached):
            two.minimize(ls, obj, 10, 50)
        assert two.k() == 10
    assert one.x().tobytes() == two.x().tobytes()
    assert two.stored_pairs() == 5 == one.stored_pairs() and two.gamma() == one.gamma()
    two.reset(x0)
    assert two.stored_pairs() == 0 and two.gamma() == 1.0 and two.resets() == 0 and two.memory == 5
    with pytest.raises(qn.MaxIterReached):
        two.minimize(ls, obj, 20, 50)
    assert one.x().tobytes() == two.x().tobytes()
    two.set_memory(3)
    assert two.memory == 3 and two.stored_pairs() == 0
    for bad in (0, 33):
        with pytest.raises(qn.ErrorInputParams):
            two.set_memory(bad)
    with pytest.raises(qn.ErrorInputParams):
        qn.solver._check(qn._abi.lib().qn_solver_set_lbfgs_memory(qn.BFGS(1e-8, [0.5, 0.5]).h, 5))
    with pytest.raises(qn.ErrorInputParams):
        qn.BFGS(1e-8, [0.5, 0.5]).set_option("lbfgs_unit_scaling", 1)
    with pytest.raises(qn.ErrorInputParams, match="More-Thuente"):
        two.minimize(qn.MoreThuente(), obj, 5, 5)
    with pytest.raises(qn.ErrorInputParams):
        two.minimize(qn.MoreThuenteB(n), obj, 5, 5)
    with pytest.raises(qn.ErrorInputParams, match="qn_minimize"):
        two.compute_direction((0.0, np.ones(n)))
    with pytest.raises(qn.ErrorInputParams):
        two.approx_inv_hessian()
    st = one.stats()
    assert st["path"] & PATH_VECTOR and st["path"] & PATH_LBFGS and st["h_passes"] == 0


def test_world_above_one_is_rejected(qn):
    from thread_ranks import run_ranks

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        with pytest.raises(qn.ErrorInputParams, match="one rank"):
            qn.LBFGS(1e-6, np.zeros(32), ctx=ctx)
        ctx.close()
        return True
    assert run_ranks(2, body, timeout=60.0) == [True, True]


def test_no_added_synchronisation(qn):
    a, c, mu, x0, _, _ = C.lse_problem(2050)
    lb, ub = C.free_box(2050)
    obj = qn.LogSumExp(a, c, mu)
    w = 20
    s, _ = _gpu(qn, obj, x0, lb, ub, "gll", 5, w)
    spg = qn.SpectralProjectedGradient(C.TOL, x0, obj, lb, ub)
    with pytest.raises(qn.MaxIterReached):
        spg.minimize(qn.GLLQuadratic(1e-4, 10), obj, w, 50)
    a_, b_ = s.stats(), spg.stats()
    assert a_["iterations"] == b_["iterations"] == w
    assert a_["host_syncs"] / a_["oracle_evals"] <= b_["host_syncs"] / b_["oracle_evals"], (a_["host_syncs"], a_["oracle_evals"], b_["host_syncs"], b_["oracle_evals"])


def test_examples_lbfgs_cpp():
    exe = os.path.join(ROOT, "examples", "lbfgs_example.bin")
    assert os.path.exists(exe), "examples/lbfgs_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "|f| < 1e-6" in p.stdout and p.stdout.strip().endswith("lbfgs example ok")
