"""GPU tests of the first-order family: QN_SPG / QN_PROJECTED_GRADIENT with GLLQuadratic and BackTrackingB through the device-wide vector
kernels (csrc/qn_vec.hip.h), against the restatement tests/ref_spg.py.  The windows (30 iterations, kappa = 1e2) and the tolerance
(1e-9 relative, as __graft_entry__.smoke() uses) are licensed case by case by the summation-order self-checks of tests/test_ref_spg.py:
the quadratic cases by test_summation_order_self_check, the device closure's and the log-sum-exp problem by the two tests beside it.
The exact check of these kernels is the step-by-step replay: tests/vec_replay.py, tests/test_gpu_vec_replay.py."""
import numpy as np
import pytest

import problems as P
import ref_spg as R
import spg_cases as S

pytestmark = pytest.mark.gpu
PATH_VECTOR = 64


def _two_var(gamma):
    def fn(x):
        return 0.5 * (x[0] ** 2 + gamma * x[1] ** 2), np.array([x[0], gamma * x[1]])
    return fn


def _gpu(qn, solver, oracle, x0, lb, ub, iters, max_ls=50, tol=1e-10, memoize=None, trace=True):
    if solver == "spg_gll":
        s = qn.SpectralProjectedGradient(tol, x0, oracle, lb, ub, memoize=memoize)
        ls = qn.GLLQuadratic(1e-4, 10)
    else:
        s = qn.ProjectedGradientDescent(tol, x0, lb, ub)
        s.memoize = memoize
        ls = qn.BackTrackingB(1e-4, 0.5, lb, ub)
    if trace:
        s.set_trace(iters, with_x=True)
    status = "ok"
    try:
        s.minimize(ls, oracle, iters, max_ls)
    except qn.MaxIterReached:
        status = "max_iter"
    return s, ls, status


def _compare(s, ref, window):
    tr, xs = s.trace()
    assert len(tr) == len(ref.trace) == window, (len(tr), len(ref.trace))
    for k in range(window):
        r = ref.trace[k]
        assert tr[k]["n_evals"] == r["n_evals"] and tr[k]["ls_iters"] == r["ls_iters"], (k, tr[k], r)
        assert abs(tr[k]["t"] - r["t"]) <= 1e-9 * abs(r["t"]), (k, tr[k]["t"], r["t"])
        assert np.linalg.norm(xs[k] - ref.trace_x[k]) <= 1e-9 * max(1.0, np.linalg.norm(ref.trace_x[k])), k
        assert abs(tr[k]["gnorm"] - r["gnorm"]) <= 1e-7 * max(1.0, r["gnorm"]), k


def test_spg_reference_test_host_closure(qn):  # spg.rs:151-204
    fn = _two_var(1e9)
    lb, ub = np.array([-1.0, 47.0]), np.array([np.inf, np.inf])
    o = R.CountingOracle(fn)
    ref = R.SpectralProjectedGradient(1e-12, [180.0, 152.0], o, lb, ub)
    ref.minimize(R.GLLQuadratic(1e-4, 10), o, 10000, 1000)
    s = qn.SpectralProjectedGradient(1e-12, [180.0, 152.0], fn, lb, ub)
    s.set_trace(10000)
    s.minimize(qn.GLLQuadratic(1e-4, 10), fn, 10000, 1000)  # Ok(())
    x = s.x()
    assert np.all(x >= lb) and np.all(x <= ub)
    assert s.has_converged(fn(x))
    tr, _ = s.trace()
    assert s.k() == ref.k == len(tr)
    assert [r["n_evals"] for r in tr] == [r["n_evals"] for r in ref.trace]
    assert s.stats()["path"] & PATH_VECTOR


def test_pgd_reference_test_host_closure(qn):  # projected_gradient_descent.rs:114-165
    fn = _two_var(999.0)
    lb, ub = np.array([-np.inf, -np.inf]), np.array([np.inf, np.inf])
    o = R.CountingOracle(fn)
    ref = R.ProjectedGradientDescent(1e-6, [180.0, 152.0], lb, ub)
    ref.minimize(R.BackTrackingB(1e-4, 0.5, lb, ub), o, 10000, 1000)
    s = qn.ProjectedGradientDescent(1e-6, [180.0, 152.0], lb, ub)
    s.set_trace(10000)
    s.minimize(qn.BackTrackingB(1e-4, 0.5, lb, ub), fn, 10000, 1000)
    x = s.x()
    assert s.has_converged(fn(x))
    tr, _ = s.trace()
    assert s.k() == ref.k == len(tr)
    assert [r["n_evals"] for r in tr] == [r["n_evals"] for r in ref.trace]
    assert s.stats()["oracle_calls"] == o.calls


@pytest.mark.parametrize("solver,n,box", S.CASES)
def test_parity_window(qn, qo, solver, n, box):
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, box)
    ref, _ = S.run_ref(solver, R.quadratic_fn(q, b), x0, lb, ub, S.WINDOW)
    obj = qn.Quadratic(q, b)
    s, _, status = _gpu(qn, solver, obj, x0, lb, ub, S.WINDOW)
    assert status == "max_iter"
    _compare(s, ref, S.WINDOW)
    assert s.stats()["path"] & PATH_VECTOR
    if solver == "spg_gll":
        assert abs(s.lambda_() - ref.lam) <= 1e-6 * ref.lam


@pytest.mark.parametrize("solver", S.SOLVERS)
@pytest.mark.parametrize("box", S.BOXES)
def test_parity_window_synthetic_4096(qn, qo, solver, box):
    n = S.BIG_N
    q, b, x0, diag = S.problem(qo, n)
    lb, ub = S.bounds(n, box)
    ref, _ = S.run_ref(solver, R.quadratic_fn(q, b), x0, lb, ub, S.WINDOW)
    obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
    s, _, _ = _gpu(qn, solver, obj, x0, lb, ub, S.WINDOW)
    _compare(s, ref, S.WINDOW)


def test_determinism_4096(qn):
    n = S.BIG_N
    diag = P.synth_diag(n, S.KAPPA)
    b, x0 = P.synth_vectors(n, P.SEED)
    lb, ub = S.bounds(n, 0.05)
    obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
    runs = []
    for _ in range(2):
        s, _, _ = _gpu(qn, "spg_gll", obj, x0, lb, ub, S.WINDOW)
        runs.append(s.trace()[1].copy())
    assert runs[0].tobytes() == runs[1].tobytes()


@pytest.mark.parametrize("solver", S.SOLVERS)
def test_device_closure_window(qn, solver):
    from test_gpu_device_closure import _Chain
    a, c, x0, lb, ub = S.chain_problem()
    ch = _Chain(qn, a, c)
    try:
        window = S.WINDOW
        ref, o = S.run_ref(solver, S.chain_fn(a, c), x0, lb, ub, window)
        s, _, _ = _gpu(qn, solver, ch.closure, x0, lb, ub, window, memoize=0)
        _compare(s, ref, window)
        assert s.stats()["total_oracle_calls"] == o.calls  # memoize = 0: the reference's sequence, the constructor's call included
        # real invocations of the closure: exactly the counted ones -- the constructor's batch stops at the loop top, and a run that ends
        # on the iteration cap ends in the post kernel (only a run that ends AT its loop top evaluates once more, unused: qn_hip.h)
        assert ch.calls() == o.calls
    finally:
        ch.close()


def test_logsumexp_window(qn):
    a, c, mu, x0, lb, ub = S.lse_problem()
    window = S.WINDOW
    ref, _ = S.run_ref("spg_gll", S.lse_fn(a, c, mu), x0, lb, ub, window)
    obj = qn.LogSumExp(a, c, mu)
    s, _, _ = _gpu(qn, "spg_gll", obj, x0, lb, ub, window)
    _compare(s, ref, window)


def test_compute_step_len_gll(qn):
    p = P.g5_ill_conditioned()
    x = np.array(p["x0"])
    f, g = p["fn"](x)
    d = -g
    o = R.CountingOracle(p["fn"])
    t_ref = R.GLLQuadratic(1e-4, 10).compute_step_len(x, (f, g), d, o, 100)
    calls = []

    def fn(xx):
        calls.append(1)
        return p["fn"](xx)
    t = qn.GLLQuadratic(1e-4, 10).compute_step_len(x, (f, g), d, fn, 100)
    assert len(calls) == o.calls
    assert abs(t - t_ref) <= 1e-12 * abs(t_ref)


def test_sync_budget_and_counters(qn, qo):
    n = 2048
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, 0.05)
    obj = qn.Quadratic(q, b)
    s = qn.SpectralProjectedGradient(1e-10, x0, obj, lb, ub)
    s.set_trace(S.WINDOW)
    before = s.stats()["host_syncs"]
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.GLLQuadratic(1e-4, 10), obj, S.WINDOW, 50)
    st = s.stats()
    tr, _ = s.trace()
    extra = sum(r["ls_iters"] - 1 for r in tr)
    # one synchronisation per iteration whose first trial is accepted, one more per further trial, and a constant
    assert st["host_syncs"] - before <= S.WINDOW + extra + 2, (st["host_syncs"] - before, extra)
    assert st["path"] & PATH_VECTOR and st["iterations"] == S.WINDOW
    # memoize = 0 on a host closure: every call of the reference's sequence is made, the constructor's included
    fn = R.quadratic_fn(q, b)
    ref, o = S.run_ref("spg_gll", fn, x0, lb, ub, S.WINDOW)
    calls = []

    def counted(x):
        calls.append(1)
        return fn(x)
    s2 = qn.SpectralProjectedGradient(1e-10, x0, counted, lb, ub)
    with pytest.raises(qn.MaxIterReached):
        s2.minimize(qn.GLLQuadratic(1e-4, 10), counted, S.WINDOW, 50)
    assert s2.stats()["total_oracle_calls"] == o.calls == len(calls)


def test_memory_is_linear_in_n(qn):
    import torch
    n = 1 << 22
    x0 = np.zeros(n)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    x0[:] = 0.5
    calls = []

    def fn(x):  # f = 1/2 ||x||^2
        calls.append(1)
        return 0.5 * float(x @ x), x
    # the SPG constructor runs the oracle once (lambda0): whatever a first evaluation allocates lazily is inside the measurement
    s = qn.SpectralProjectedGradient(1e-6, x0, fn, np.full(n, -1.0), np.full(n, 1.0))
    assert len(calls) == 1 and s.lambda_() == 2.0  # clamp(1 / ||P(x0 - g0) - x0||_inf) = 1 / 0.5
    free1, _ = torch.cuda.mem_get_info()
    # 9 work vectors + 3 of mat-vec scratch + 4 of bounds = 16 n doubles; 24 leaves room for the allocator's granularity.
    # (An n x n matrix would be 2^22 n doubles.)
    assert free0 - free1 <= 24 * n * 8, (free0 - free1) / (n * 8)
    with pytest.raises(qn.ErrorInputParams):
        s.approx_inv_hessian()
    with pytest.raises(qn.ErrorInputParams):
        s.set_approx_inv_hessian(np.eye(2))
    s.close()


def test_rejections(qn):
    fn = _two_var(10.0)
    lb, ub = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    s = qn.SpectralProjectedGradient(1e-8, [0.5, 0.5], fn, lb, ub)
    with pytest.raises(qn.ErrorInputParams, match="More-Thuente"):
        s.minimize(qn.MoreThuente(), fn, 5, 5)
    with pytest.raises(qn.ErrorInputParams):
        s.minimize(qn.MoreThuenteB(2), fn, 5, 5)
    for m in (0, 65):
        with pytest.raises(qn.ErrorInputParams):
            s.minimize(qn.GLLQuadratic(1e-4, m), fn, 5, 5)
    with pytest.raises(qn.ErrorInputParams, match="GLLQuadratic"):
        qn.BFGS(1e-8, [0.5, 0.5]).minimize(qn.GLLQuadratic(1e-4, 10), fn, 5, 5)
    with pytest.raises(qn.ErrorInputParams):
        s.secant_update(np.ones(2), np.ones(2))
    p = qn.ProjectedGradientDescent(1e-8, [0.5, 0.5], lb, ub)
    with pytest.raises(qn.ErrorInputParams):
        qn.solver._check(qn._abi.lib().qn_solver_set_spg_lambdas(p.h, 1e-2, 1e2))
    # compute_direction: P(x - lambda g) - x with the current lambda (spg.rs:76-86)
    lam = s.lambda_()
    g = np.array([3.0, -100.0])
    x = s.x()
    assert np.array_equal(s.compute_direction((0.0, g)), np.minimum(np.maximum(x - lam * g, lb), ub) - x)
    assert np.array_equal(p.compute_direction((0.0, g)), np.minimum(np.maximum(p.x() - g, lb), ub) - p.x())
    s.with_lambdas(1e-2, 1e2)
    assert (s.lambda_min(), s.lambda_max()) == (1e-2, 1e2) and s.lambda_() == lam


def test_world_above_one_is_rejected(qn):
    """One rank only: on a context of a 2-rank group the two solvers cannot be created (ranks as threads, as tests/test_gpu_partitions.py)."""
    from thread_ranks import run_ranks

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        seen = []
        for cls, args in ((qn.ProjectedGradientDescent, ()), (qn.SpectralProjectedGradient, (lambda x: (0.0, x),))):
            with pytest.raises(qn.ErrorInputParams, match="one rank"):
                cls(1e-6, np.zeros(32), *args, -np.ones(32), np.ones(32), ctx=ctx)
            seen.append(cls.__name__)
        qn.GradientDescent(1e-6, np.zeros(32), ctx=ctx).close()  # (the context itself is fine)
        ctx.close()
        return seen
    assert run_ranks(2, body, timeout=60.0) == [["ProjectedGradientDescent", "SpectralProjectedGradient"]] * 2


def test_reset_projects_x0(qn):
    lb, ub = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    p = qn.ProjectedGradientDescent(1e-8, [0.5, 0.5], lb, ub)
    p.reset(np.array([3.0, -0.25]))
    assert np.array_equal(p.x(), [1.0, -0.25])  # ::new projects x0 (spg.rs:35, projected_gradient_descent.rs:21)
    n = 1 << 20  # large enough that the upload is not over before the next call is made
    big = qn.ProjectedGradientDescent(1e-8, np.zeros(n), np.full(n, -1.0), np.full(n, 1.0))
    x0 = np.linspace(-3.0, 3.0, n)
    big.reset(x0)
    assert np.array_equal(big.x(), np.clip(x0, -1.0, 1.0))


def test_spg_example_cpp():
    """examples/spg_example.cpp: the reference's examples/spg_example.rs problem through the C++ mirror (include/qn_solver.hpp)."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "spg_example.bin")
    assert os.path.exists(exe), "examples/spg_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("spg example ok")


def test_warm_restart_bit_for_bit(qn, qo):
    n = 512
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, 0.05)
    obj = qn.Quadratic(q, b)
    one, _, _ = _gpu(qn, "spg_gll", obj, x0, lb, ub, 30)
    two = qn.SpectralProjectedGradient(1e-10, x0, obj, lb, ub)
    ls = qn.GLLQuadratic(1e-4, 10)
    for _ in range(2):
        with pytest.raises(qn.MaxIterReached):
            two.minimize(ls, obj, 15, 50)
        assert two.k() == 15
    assert one.x().tobytes() == two.x().tobytes()
    assert one.lambda_() == two.lambda_()
    # reset: no lambda, an empty history
    two.reset(x0)
    assert two.lambda_() is None
