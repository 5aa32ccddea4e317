"""GPU tests of QN_OWLQN (qn.OWLQN; kernels csrc/qn_vec_owlqn.hip.h) against the restatement tests/ref_owlqn.py and the rules of DESIGN.md
section 35: the pseudo-gradient, the alignment and the projected point bit for bit at every iteration; the first iteration bit for bit at
n <= 2; windows and whole runs against the restatement and against SpectralProximalGradient; state across calls and set_l1; the
synchronisation budget, the path, the memory and the refusals."""
import math

import numpy as np
import pytest

import logistic_cases as LC
import owlqn_cases as OC
import prox_cases as PC
import ref_owlqn as RO
import sparse_cases as SC
import spg_cases as S
from test_gpu_prox import _device_objective, _Window
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
PATH_VECTOR, PATH_LBFGS, PATH_OWLQN = 64, 1024, 32768
PATHS = PATH_VECTOR | PATH_LBFGS | PATH_OWLQN
SIZES = (1, 2, 3, 255, 256, 257, 1000, 4099)


def _bt(qn):
    return qn.BackTracking(OC.C1, OC.BETA)


def _run(qn, s, oracle, iters, max_ls=OC.MAX_LS, callback=None):
    try:
        s.minimize(_bt(qn), oracle, iters, max_ls, callback=callback)
    except qn.MaxIterReached:
        return "max_iter"
    return "ok"


# ---- 1. the element-wise rules, bit for bit ----
def _crafted(n, l1vec):
    """f = 1/2 sum q_j (x_j - c_j)^2 with q_j <= 1 (so the first search accepts t = 1) and, by j mod 8: 0 x_j == 0 with |g_j| <= l1_j: stays;
    1 x_j == 0 with |g_j| > l1_j: leaves; 2 crosses zero at t = 1: projected onto 0.0; 3 unpenalised (vector l1) and crossing zero freely;
    4 .. 7 generic.  The scalar penalty is 0.25: kinds 0 to 2 keep their behaviour, kind 3 is then penalised and behaves as kind 2."""
    rng = np.random.default_rng(300 + n)
    j = (np.arange(n) + 4) % 8  # (n < 5: generic entries only)
    x0, c, q = rng.uniform(-0.4, 0.4, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0.5, 1.0, n)
    l1 = rng.uniform(0.05, 0.3, n)
    for k, (xv, cv, qv, lv) in {0: (0.0, 0.125, 1.0, 0.25), 1: (0.0, 1.0, 1.0, 0.25), 2: (0.1, -1.0, 1.0, 0.25), 3: (0.1, -1.0, 1.0, 0.0)}.items():
        x0[j == k], c[j == k], q[j == k], l1[j == k] = xv, cv, qv, lv
    if not l1vec:
        l1 = np.full(n, 0.25)

    def fn(x):
        return 0.5 * float(np.sum(q * (x - c) ** 2)), q * (x - c)
    return fn, x0, (l1 if l1vec else 0.25), l1


def _check_rules(qn, s, oracle, x0, g0, l1, iters):
    """run `iters` iterations; at every one, from the solver's own (x_k, g_k): v_k, the trace's gnorm, the signs of d_k, and x_{k+1} by rule 5"""
    seen = []

    def cb(sv):
        seen.append((sv.pseudo_gradient(), sv.direction(), sv.x(), sv.gradient()))
    s.set_trace(iters, with_x=True)
    _run(qn, s, oracle, iters, callback=cb)
    tr, xs = s.trace()
    assert len(tr) == len(seen) >= 1
    x_k, g_k = x0, g0
    for k, (v_k, d_k, x_next, g_next) in enumerate(seen):
        want = RO.pseudo_gradient(x_k, g_k, l1)
        assert v_k.tobytes() == want.tobytes(), (k, np.flatnonzero(v_k != want)[:5])
        assert tr[k]["gnorm"] == float(np.max(np.abs(v_k))), k
        pen = (l1 > 0.0) & (d_k != 0.0)
        assert np.all(np.sign(d_k[pen]) == -np.sign(v_k[pen])), k
        assert not np.any(np.signbit(d_k[(d_k == 0.0) & (l1 > 0.0)])), k
        xt = RO.project(x_k, d_k, v_k, l1, tr[k]["t"])
        assert x_next.tobytes() == xt.tobytes() == xs[k].tobytes(), (k, np.flatnonzero(x_next != xt)[:5])
        assert not np.any(np.signbit(x_next[x_next == 0.0])), k  # exact zeros are the literal 0.0
        x_k, g_k = x_next, g_next
    return seen, tr


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("l1vec", [False, True])
def test_element_rules_bit_for_bit(qn, n, l1vec):
    fn, x0, l1_arg, l1 = _crafted(n, l1vec)
    s = qn.OWLQN(1e-300, x0, l1_arg, memoize=1)
    try:
        g0 = fn(x0)[1]
        seen, tr = _check_rules(qn, s, fn, x0, g0, l1, 6)
        if n >= 8:  # the data holds what the rules are about
            j = (np.arange(n) + 4) % 8
            v0, d0, x1 = seen[0][0], seen[0][1], seen[0][2]
            assert tr[0]["t"] == 1.0 and tr[0]["ls_iters"] == 1
            assert np.all(v0[j == 0] == 0.0) and np.all(d0[j == 0] == 0.0) and np.all(x1[j == 0] == 0.0)  # at 0 with |g| <= l1: stays
            assert np.all(x0[j == 1] == 0.0) and np.all(x1[j == 1] == 0.75)                                 # at 0 with |g| > l1: leaves
            assert np.all(x0[j == 2] + d0[j == 2] < 0.0) and np.all(x1[j == 2] == 0.0)                      # crosses zero: 0.0
            if l1vec:
                assert np.all(l1[j == 3] == 0.0) and np.all(x1[j == 3] == x0[j == 3] + d0[j == 3]) and np.all(x1[j == 3] < 0.0)  # smooth: crosses freely
            assert len(seen) >= 4
        st = s.stats()
        assert st["path"] & PATHS == PATHS
    finally:
        s.close()


def test_element_rules_past_one_grid_trip(qn):
    """n = 2^20 + 3 on a tridiagonal SparseQuadratic, 4 iterations: every thread of the four streaming kernels takes more than one trip of the
    grid-stride loop (1024 workgroups x 256 threads x 2 entries = 2^19 per trip), the last trip ragged"""
    n = (1 << 20) + 3
    indptr, cols, vals = SC.tri(n)
    obj = qn.SparseQuadratic(indptr, cols, vals, SC.rhs(n))
    x0 = SC.start(n) - 1.0  # [-0.5, 0.5)
    x0[::11] = 0.0
    l1 = np.full(n, 0.3)
    l1[::5] = 0.0
    s = qn.OWLQN(1e-300, x0, l1)
    try:
        g0 = np.asarray(obj(x0).g(), dtype=np.float64)
        seen, tr = _check_rules(qn, s, obj, x0, g0, l1, 4)
        assert len(seen) == 4
        x = seen[-1][2]
        assert np.any(x == 0.0) and np.any(x[l1 == 0.0] != 0.0) and s.stored_pairs() >= 1
    finally:
        s.close()
        obj.close()


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_first_iteration_bit_for_bit(qn, n):
    """n <= 2: every sum has one order and the first iteration has no pair (z = v), so F_k, the measure, t, the counts and x are the restatement's
    with ref_prox.seq_dot, bit for bit.  (The comparison that rejects Armijo's right side: tests/test_ref_owlqn.py::test_planted_fault_armijo_right_side.)"""
    ref = OC.run_tiny(n)
    fn, x0, l1 = OC.tiny_problem(n)
    s = qn.OWLQN(1e-12, x0, l1)
    try:
        s.set_trace(1, with_x=True)
        assert _run(qn, s, fn, 1) == "max_iter"
        tr, xs = s.trace()
        assert len(tr) == len(ref.trace) == 1
        for key in ("f", "gnorm", "t", "n_evals", "ls_iters", "s_norm", "updated"):
            assert tr[0][key] == ref.trace[0][key], (key, tr[0][key], ref.trace[0][key])
        assert xs[0].tobytes() == ref.trace_x[0].tobytes() and xs[0][0] == 0.0
        assert s.direction().tobytes() == ref.trace_d[0].tobytes() and s.pseudo_gradient().tobytes() == ref.trace_v[0].tobytes()
    finally:
        s.close()


# ---- 3. windows against the restatement ----
@pytest.mark.parametrize("kind,shape,m", OC.WINDOW_CASES)
@pytest.mark.parametrize("memoize", [0, 1])
def test_window_against_ref_owlqn(qn, qo, kind, shape, m, memoize):
    w = OC.WINDOWS[(kind, shape, m)]
    ref = OC.run_ref(kind, shape, m, qo)[0]
    obj = _device_objective(qn, qo, kind, shape)
    _, x0 = PC.smooth(kind, shape, qo)
    s = qn.OWLQN(OC.TOL, x0, OC.l1_of(kind, shape), m=m, memoize=memoize)
    try:
        s.set_trace(w, with_x=True)
        assert _run(qn, s, obj, w) == "max_iter"
        _compare(s, _Window(ref, w), w)
        tr, xs = s.trace()
        for k in range(w):
            assert abs(tr[k]["f"] - ref.trace[k]["f"]) <= 1e-9 * max(1.0, abs(ref.trace[k]["f"])), k  # F_k = f + h0
            assert tr[k]["updated"] == ref.updated[k], k
        assert np.array_equal(xs[w - 1] == 0.0, ref.trace_x[w - 1] == 0.0)  # the zero pattern at the window's end
        assert 0 < np.count_nonzero(xs[w - 1]) < x0.size
        assert s.stats()["path"] & PATHS == PATHS
    finally:
        s.close()
        obj.close()


# ---- 4. whole runs ----
def _whole_oracle(qn, kind, m, n, device):
    fn, l1, x0 = PC.run_problem(kind, m, n)
    if not device:
        return fn, fn, l1, x0, lambda: None
    a, y, w, _, _, _ = LC.problem(m, n)
    if kind == "logistic":
        obj = qn.Logistic(a, y, PC.RUN_MU, weights=w)
    else:  # 1/2 ||A x - b||^2 + mu/2 ||x||^2 = 1/2 x'(A'A + mu I)x - (A'b)'x + const; A'b = -g(0)
        obj = qn.Quadratic(a.T @ a + PC.RUN_MU * np.eye(n), -fn(np.zeros(n))[1])
    return obj, fn, l1, x0, obj.close


@pytest.mark.parametrize("kind,m,n", OC.RUN_CASES)
@pytest.mark.parametrize("device", [False, True])
def test_whole_run(qn, kind, m, n, device):
    """The GPU run converges to RUN_TOL within the restatement's own iteration count plus 10 % (rounded up), to the restatement's zero pattern; a GPU
    SpectralProximalGradient + GLLQuadratic(1e-4, 10) run to the same tolerance gives the same zero pattern and an x within ten times the
    CPU-recorded |x_owlqn - x_prox| (owlqn_cases.RUN_GAP: the two stopping points lie at different places inside the same tolerance ball)."""
    ref, status = OC.run_whole(kind, m, n)
    assert status == "ok"
    oracle, fn, l1, x0, close = _whole_oracle(qn, kind, m, n, device)
    cap = int(math.ceil(1.1 * len(ref.trace)))
    s = qn.OWLQN(OC.RUN_TOL, x0, l1)
    p = qn.SpectralProximalGradient(OC.RUN_TOL, x0, oracle, l1)
    try:
        status = _run(qn, s, oracle, cap)
        x = s.x()
        print(f"whole run {kind} ({m}, {n}) device={device}: restatement {len(ref.trace)} iterations, GPU {s.k()} ({status}); nonzeros {s.nonzeros()} / {np.count_nonzero(ref.x)}; "
              f"evaluations {s.stats()['oracle_evals']}")
        assert status == "ok", (s.k(), len(ref.trace))
        assert np.array_equal(x == 0.0, ref.x == 0.0)
        assert s.has_converged(fn(x))
        p.minimize(qn.GLLQuadratic(1e-4, 10), oracle, PC.RUN_CAP, PC.MAX_LS)
        xp = p.x()
        gap = float(np.max(np.abs(x - xp)))
        print(f"    SpectralProximalGradient: {p.k()} iterations, evaluations {p.stats()['oracle_evals']}, |x_owlqn - x_prox| = {gap:.3e} (CPU-recorded {OC.RUN_GAP:.3e})")
        assert np.array_equal(xp == 0.0, x == 0.0)
        assert gap <= 10.0 * OC.RUN_GAP
    finally:
        s.close()
        p.close()
        close()


# ---- 5. state across calls ----
def _state_problem(qn, qo):
    n = 512
    q, b, x0, _ = S.problem(qo, n)
    l1 = np.full(n, 0.4)
    l1[::3] = 0.0
    return qn.Quadratic(q, b), x0, l1


def test_two_calls_are_one(qn, qo):
    obj, x0, l1 = _state_problem(qn, qo)
    try:
        one = qn.OWLQN(1e-10, x0, l1)
        one.set_trace(24, with_x=True)
        assert _run(qn, one, obj, 24) == "max_iter"
        two = qn.OWLQN(1e-10, x0, l1)
        xs2, tr2 = [], []
        for _ in range(2):
            two.set_trace(12, with_x=True)
            assert _run(qn, two, obj, 12) == "max_iter" and two.k() == 12
            tr, xs = two.trace()
            tr2 += tr
            xs2.append(xs)
        tr1, xs1 = one.trace()
        assert xs1.tobytes() == np.concatenate(xs2).tobytes() and tr1 == tr2
        assert one.x().tobytes() == two.x().tobytes() and one.gamma() == two.gamma() and one.stored_pairs() == two.stored_pairs() == 5
        assert one.resets() == two.resets()
        two.reset(x0)
        assert two.stored_pairs() == 0 and np.array_equal(two.l1, l1)  # the penalty is a setting: kept
        one.close()
        two.close()
    finally:
        obj.close()


def test_fresh_runs_give_identical_bytes(qn, qo):
    obj, x0, l1 = _state_problem(qn, qo)
    try:
        out = []
        for _ in range(2):
            s = qn.OWLQN(1e-10, x0, l1)
            s.set_trace(20, with_x=True)
            assert _run(qn, s, obj, 20) == "max_iter"
            tr, xs = s.trace()
            out.append((s.x().tobytes(), xs.tobytes(), tr))
            s.close()
        assert out[0] == out[1]
    finally:
        obj.close()


def test_set_l1_keeps_the_pairs_and_the_memo(qn):
    """the regularisation path on logistic (96, 64): l1 2 -> 1 after 6 iterations.  The pairs are differences of the smooth gradient and stay; x and
    the memoised evaluation stay (no evaluation at x in the next call); set_lbfgs_memory empties the memory"""
    (a, y, w, mu), fn, x0 = OC.restart_problem()
    obj = qn.Logistic(a, y, mu, weights=w)
    s = qn.OWLQN(OC.RUN_TOL, x0, OC.RESTART_L1[0])
    try:
        assert _run(qn, s, obj, OC.RESTART_K) == "max_iter"
        stored, x, gam = s.stored_pairs(), s.x(), s.gamma()
        assert stored == 5
        s.set_l1(OC.RESTART_L1[1])
        assert s.stored_pairs() == stored and s.x().tobytes() == x.tobytes() and np.all(s.l1 == OC.RESTART_L1[1])
        s.set_trace(3)
        assert _run(qn, s, obj, 3) == "max_iter"
        tr, _ = s.trace()
        st = s.stats()
        # every call of the sequence that found its point evaluated: the loop top and the accepted point of every iteration -- the first loop top among
        # them, which a call without the memo has to evaluate
        assert st["oracle_calls"] - st["oracle_evals"] == 2 * 3
        assert st["oracle_evals"] == sum(r["ls_iters"] for r in tr)
        assert abs(tr[0]["f"] - (obj(x).f() + OC.RESTART_L1[1] * np.sum(np.abs(x)))) <= 1e-12 * abs(tr[0]["f"])  # F_k at the NEW penalty from the kept smooth f
        assert s.stored_pairs() == 5 and s.gamma() != gam
        s.set_x(s.x())  # drops the memo: the same call now pays for its first loop top
        assert _run(qn, s, obj, 2) == "max_iter"
        st = s.stats()
        assert st["oracle_calls"] - st["oracle_evals"] == 2 * 2 - 1
        s.set_memory(3)
        assert s.stored_pairs() == 0 and s.memory == 3
        s.minimize(_bt(qn), obj, 2000, OC.MAX_LS)  # Ok(()): converged at the new penalty
        assert s.has_converged(obj(s.x())) and 0 < s.nonzeros() < s.n and s.stored_pairs() == 3
    finally:
        s.close()
        obj.close()


# ---- 6. budget and bookkeeping ----
def test_sync_budget_and_path(qn, qo):
    n, window = 2048, 30
    q, b, x0, _ = S.problem(qo, n)
    obj = qn.Quadratic(q, b)
    s = qn.OWLQN(1e-10, x0, 0.2)
    try:
        s.set_trace(window)
        before = s.stats()["host_syncs"]
        assert _run(qn, s, obj, window) == "max_iter"
        st = s.stats()
        tr, _ = s.trace()
        extra = sum(r["ls_iters"] - 1 for r in tr)
        assert st["host_syncs"] - before <= window + extra + 2, (st["host_syncs"] - before, extra)
        assert st["path"] == PATHS and st["iterations"] == window
    finally:
        s.close()
        obj.close()


def test_one_vector_beyond_lbfgs(qn):
    import torch
    n = 1 << 22

    def fn(x):  # f = 1/2 ||x - 1||^2
        return 0.5 * float((x - 1.0) @ (x - 1.0)), x - 1.0
    used = []
    for make in (lambda: qn.LBFGS(1e-6, np.full(n, 0.5)), lambda: qn.OWLQN(1e-6, np.full(n, 0.5), 0.25)):
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        s = make()
        try:
            s.minimize(_bt(qn), fn, 1, 5)
        except qn.MaxIterReached:
            pass
        free1, _ = torch.cuda.mem_get_info()
        used.append(free0 - free1)
        s.close()
    # the pseudo-gradient's n_pad doubles and three scalars; a quarter of a vector for the allocator's granularity
    assert used[1] - used[0] <= 1.25 * n * 8, (used[1] - used[0]) / (n * 8)
    assert used[1] <= 32 * n * 8  # (an n x n matrix would be 2^22 n)


# ---- 7. refusals, each before any launch ----
def test_refusals(qn):
    def fn(x):
        return 0.5 * float(x @ x), x
    x0 = np.array([0.5, -0.25, 0.125])
    lb, ub = -np.ones(3), np.ones(3)
    s = qn.OWLQN(1e-8, x0, 0.1)
    lb5 = qn.LBFGS(1e-8, x0)
    L = qn._abi.lib()
    try:
        assert _run(qn, s, fn, 1) == "max_iter"
        launches, x = s.stats()["launches"], s.x()
        for ls in (qn.GLLQuadratic(1e-4, 10), qn.StrongWolfe(), qn.BackTrackingB(1e-4, 0.5, lb, ub), qn.ExactQuadratic(), qn.MoreThuente(), qn.MoreThuenteB(3), qn.NoSearch()):
            with pytest.raises(qn.ErrorInputParams):
                s.minimize(ls, fn, 5, 5)
        with pytest.raises(qn.ErrorInputParams):
            s.compute_direction((0.0, np.ones(3)))
        for bad in (-1.0, float("nan"), float("inf"), np.array([0.1, -0.1, 0.1]), np.array([0.1, np.nan, 0.1]), np.array([0.1, np.inf, 0.1]), np.ones(2)):
            with pytest.raises(qn.ErrorInputParams):
                s.set_l1(bad)
        assert np.all(s.l1 == 0.1)
        out = np.empty(3)
        with pytest.raises(qn.ErrorInputParams):  # pseudo_gradient() on another method
            qn.solver._check(L.qn_solver_get_pseudo_gradient(lb5.h, out.ctypes.data_as(qn._abi.dp)))
        with pytest.raises(qn.ErrorInputParams):
            qn.solver._check(L.qn_solver_get_pseudo_gradient(None, out.ctypes.data_as(qn._abi.dp)))
        with pytest.raises(qn.ErrorInputParams):
            s.set_memory(33)
        assert s.stats()["launches"] == launches and s.x().tobytes() == x.tobytes()
        # a box: refused by the run, before any launch
        boxed = qn.OWLQN(1e-8, x0, 0.1)
        qn.solver._check(L.qn_solver_set_bounds(boxed.h, lb.ctypes.data_as(qn._abi.dp), ub.ctypes.data_as(qn._abi.dp)))
        with pytest.raises(qn.ErrorInputParams):
            boxed.minimize(_bt(qn), fn, 5, 5)
        assert boxed.stats()["launches"] == 0
        boxed.close()
        # a solver that has not run yet: nothing was ever launched
        raw = qn.OWLQN(1e-8, x0, 0.1)
        with pytest.raises(qn.ErrorInputParams):
            raw.minimize(qn.StrongWolfe(), fn, 5, 5)
        assert raw.stats()["launches"] == 0
        raw.set_option("lbfgs_unit_scaling", 1)  # accepted
        raw.close()
    finally:
        s.close()
        lb5.close()


def test_not_a_descent_direction_ends_the_run(qn):
    """rule 3: a v.d that is not finite (the closure's gradient is +inf in its smooth entry from the second iteration on while f stays finite; a NaN
    there would count as a stationary entry under rule 1, as under DESIGN 34's measure) ends the run with AbnormalTermination and leaves x at x_k"""
    calls = []
    q = np.array([1.0, 2.0, 3.0])

    def fn(x):
        calls.append(1)
        g = q * (x - 1.0)
        if len(calls) > 3:
            g[1] = np.inf
        return 0.5 * float(np.sum(q * (x - 1.0) ** 2)), g
    s = qn.OWLQN(1e-12, np.array([0.5, -0.25, 0.125]), np.array([0.1, 0.0, 0.1]))  # (entry 1 is smooth: v_1 = g_1)
    try:
        with pytest.raises(qn.AbnormalTermination, match="not a descent direction"):
            s.minimize(_bt(qn), fn, 10, 5)
        assert np.all(np.isfinite(s.x()))
    finally:
        s.close()


def test_world_above_one_is_rejected(qn):
    from thread_ranks import run_ranks

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        with pytest.raises(qn.ErrorInputParams, match="one rank"):
            qn.OWLQN(1e-6, np.zeros(32), 0.1, ctx=ctx)
        ctx.close()
        return True
    assert run_ranks(2, body, timeout=60.0) == [True, True]
