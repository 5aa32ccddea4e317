"""GPU tests of QN_PROJECTED_NEWTON / QN_SPECTRAL_PROJECTED_NEWTON (csrc/qn_vec.hip.h's phase machine with the Cholesky solve of
csrc/qn_host_newton.hip.h) against the restatement tests/ref_pnewton.py.  The windows (30 iterations, kappa = 1e2, GLLQuadratic(1e-4, 10),
tol 1e-10) and the 1e-9 relative tolerance are licensed case by case by tests/test_ref_pnewton.py's summation-order self-checks.

ProjectedNewton's s_norm / y_norm in the trace get bounds that follow from the 1e-9 on x: s = x_next - x differs by at most
2e-9 max(1, ||x||), and y = g(x_next) - g(x) by at most L times that, L a bound on the Hessian's norm (its largest absolute row sum for the
quadratic, ||A||_2^2 + mu for the log-sum-exp problem).
The exact check of these kernels is the step-by-step replay: tests/vec_replay.py, tests/test_gpu_vec_replay.py."""
import ctypes as C

import numpy as np
import pytest

import pnewton_cases as PC
import problems as P
import ref_pnewton as RP
import ref_spg as R
import spg_cases as S
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
PATH_VECTOR, PATH_PNEWTON = 64, 128


def _two_var(gamma):
    h = np.array([[1.0, 0.0], [0.0, gamma]])

    def fn(x):
        return 0.5 * (x[0] ** 2 + gamma * x[1] ** 2), np.array([x[0], gamma * x[1]]), h
    return fn


def _gpu(qn, solver, oracle, x0, lb, ub, iters, max_ls=50, tol=PC.TOL, memoize=None, reuse=None, callback=None):
    if solver == "spn":
        s = qn.SpectralProjectedNewton(tol, x0, oracle, lb, ub, memoize=memoize)
    else:
        s = qn.ProjectedNewton(tol, x0, lb, ub)
        s.memoize = memoize
    if reuse is not None:
        s.set_option("pnewton_reuse_factor", reuse)
    s.set_trace(iters, with_x=True)
    status = "ok"
    try:
        s.minimize(qn.GLLQuadratic(1e-4, 10), oracle, iters, max_ls, callback)
    except qn.MaxIterReached:
        status = "max_iter"
    return s, status


def _compare_norms(s, ref, lip):
    tr, _ = s.trace()
    for k, r in enumerate(tr):
        scale = 2e-9 * max(1.0, float(np.linalg.norm(ref.trace_x[k])))
        assert abs(r["s_norm"] - ref.trace[k]["s_norm"]) <= scale, (k, r["s_norm"], ref.trace[k]["s_norm"])
        assert abs(r["y_norm"] - ref.y_norms[k]) <= lip * scale, (k, r["y_norm"], ref.y_norms[k])


def _check_case(qn, solver, oracle, fn, x0, lb, ub, lip, window=PC.WINDOW):
    ref, o, rstatus = PC.run_ref(solver, fn, x0, lb, ub, window)
    s, status = _gpu(qn, solver, oracle, x0, lb, ub, window)
    assert status == rstatus
    _compare(s, ref, len(ref.trace))
    st = s.stats()
    assert st["path"] & PATH_VECTOR and st["path"] & PATH_PNEWTON
    if solver == "spn":
        assert abs(s.lambda_() - ref.lam) <= 1e-6 * ref.lam
    else:
        _compare_norms(s, ref, lip)
        assert s.next_iterate_too_close() == ref.next_iterate_too_close()
        assert s.gradient_next_iterate_too_close() == ref.gradient_next_iterate_too_close()
    return s, ref, o


def test_projected_newton_reference_test_host_closure(qn):  # projected_newton.rs:147-198
    fn = _two_var(90.0)
    lb, ub = np.array([-np.inf, -np.inf]), np.array([np.inf, np.inf])
    o = RP.HessianOracle(fn)
    ref = RP.ProjectedNewton(1e-6, [180.0, 152.0], lb, ub)
    ref.minimize(R.GLLQuadratic(1e-4, 15), o, 10000, 1000)
    s = qn.ProjectedNewton(1e-6, [180.0, 152.0], lb, ub)
    s.set_trace(100, with_x=True)
    s.minimize(qn.GLLQuadratic(1e-4, 15), fn, 10000, 1000)  # Ok(())
    assert s.has_converged(fn(s.x()))
    tr, xs = s.trace()
    assert s.k() == ref.k == len(tr)
    assert [r["n_evals"] for r in tr] == [r["n_evals"] for r in ref.trace]
    assert [r["t"] for r in tr] == [r["t"] for r in ref.trace]
    assert xs.tobytes() == np.array(ref.trace_x).tobytes()  # n = 2: nalgebra's operation order, decision for decision and bit for bit
    assert s.s_norm() == ref.s_norm and s.y_norm() == ref.y_norm
    assert s.stats()["oracle_calls"] == o.calls
    assert s.stats()["path"] & PATH_PNEWTON


def test_spectral_projected_newton_reference_test_host_closure(qn):  # spn.rs:155-210
    fn = _two_var(1e9)
    lb, ub = np.array([-1.0, 47.0]), np.array([np.inf, np.inf])
    o = RP.HessianOracle(fn)
    ref = RP.SpectralProjectedNewton(1e-12, [180.0, 152.0], o, lb, ub)
    ref.minimize(R.GLLQuadratic(1e-4, 10), o, 10000, 1000)
    s = qn.SpectralProjectedNewton(1e-12, [180.0, 152.0], fn, lb, ub)
    s.set_trace(10000, with_x=True)
    s.minimize(qn.GLLQuadratic(1e-4, 10), fn, 10000, 1000)  # Ok(())
    x = s.x()
    assert np.all(x >= lb) and np.all(x <= ub) and s.has_converged(fn(x))
    tr, xs = s.trace()
    assert s.k() == ref.k == len(tr)
    assert [(r["n_evals"], r["ls_iters"], r["t"]) for r in tr] == [(r["n_evals"], r["ls_iters"], r["t"]) for r in ref.trace]
    assert xs.tobytes() == np.array(ref.trace_x).tobytes()
    assert s.lambda_() == ref.lam
    assert s.stats()["total_oracle_calls"] == o.calls  # the constructor's call included


@pytest.mark.parametrize("solver,n,box", PC.QUAD_CASES)
def test_parity_window_quadratic(qn, qo, solver, n, box):
    """n = 64 and 512: 64-wide triangular blocks; n = 1000: the 512-wide ones (newton_big), not a multiple of 64."""
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, box)
    lip = float(np.max(np.sum(np.abs(q), axis=1)))
    s, ref, _ = _check_case(qn, solver, qn.Quadratic(q, b), RP.quadratic_fn(q, b), x0, lb, ub, lip)
    if solver == "pn":  # ends after 1-2 iterations: by the gradient test in the infinite box, by s_norm in +-0.05
        assert ref.ended_by == ("projected_gradient" if np.isinf(box) else "s_norm")
        if not np.isinf(box):
            assert s.next_iterate_too_close()
            assert not float(np.max(np.abs(s.projected_gradient(RP.quadratic_fn(q, b)(s.x()))))) < PC.TOL
    else:
        assert len(ref.trace) == PC.WINDOW


@pytest.mark.parametrize("solver,box", PC.LSE_CASES)
def test_parity_window_logsumexp_host_closure(qn, solver, box):
    a, c, mu, x0, _, _ = S.lse_problem()
    lb, ub = S.bounds(x0.size, box)
    fn = PC.lse_hess_fn(a, c, mu)
    lip = float(np.linalg.norm(a, 2) ** 2 + mu)
    s, ref, o = _check_case(qn, solver, fn, fn, x0, lb, ub, lip)
    assert s.newton_factorisations() == len(ref.trace)  # a host closure: one factorisation per direction
    assert s.stats()["total_oracle_calls"] == o.calls  # memoize = 0: the reference's call sequence (the constructor's call included)


@pytest.mark.parametrize("solver", PC.SOLVERS)
def test_device_quadratic_and_host_closure_agree(qn, qo, solver):
    n = 200  # not a multiple of 64
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, 0.05)
    fn = RP.quadratic_fn(q, b)
    lip = float(np.max(np.sum(np.abs(q), axis=1)))
    dev, ref, _ = _check_case(qn, solver, qn.Quadratic(q, b), fn, x0, lb, ub, lip)
    host, _, _ = _check_case(qn, solver, fn, fn, x0, lb, ub, lip)
    xd, xh = dev.trace()[1], host.trace()[1]
    assert len(xd) == len(xh)
    for k in range(len(xd)):
        assert np.linalg.norm(xd[k] - xh[k]) <= 1e-9 * max(1.0, np.linalg.norm(xh[k]))


@pytest.mark.parametrize("solver", PC.SOLVERS)
@pytest.mark.parametrize("box", PC.BOXES)
def test_parity_window_synthetic_4096(qn, qo, box, solver):
    n = PC.BIG_N
    q, b, x0, diag = S.problem(qo, n)
    lb, ub = S.bounds(n, box)
    ref, _, rstatus = PC.run_ref(solver, RP.quadratic_fn(q, b), x0, lb, ub, PC.WINDOW)
    obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
    s, status = _gpu(qn, solver, obj, x0, lb, ub, PC.WINDOW)
    assert status == rstatus and len(ref.trace) == (PC.WINDOW if solver == "spn" else len(ref.trace)) >= 1
    _compare(s, ref, len(ref.trace))
    if solver == "pn":
        _compare_norms(s, ref, float(np.max(np.sum(np.abs(q), axis=1))))
        assert s.next_iterate_too_close() == ref.next_iterate_too_close()
    assert s.newton_factorisations() == 1


def test_determinism_and_factor_reuse_4096(qn):
    n = PC.BIG_N
    diag = P.synth_diag(n, S.KAPPA)
    b, x0 = P.synth_vectors(n, P.SEED)
    lb, ub = S.bounds(n, 0.05)
    obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
    runs = []
    for reuse in (1, 1, 0):
        s, _ = _gpu(qn, "spn", obj, x0, lb, ub, PC.WINDOW, reuse=reuse)
        runs.append(s.trace()[1].copy())
        assert s.newton_factorisations() == (1 if reuse else PC.WINDOW)
        s.close()
    assert runs[0].tobytes() == runs[1].tobytes()  # run to run
    assert runs[0].tobytes() == runs[2].tobytes()  # the kept factor against factorising in every iteration


@pytest.mark.parametrize("solver", PC.SOLVERS)
def test_factor_reuse_counts(qn, qo, solver):
    n = 512
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, 0.05)
    obj = qn.Quadratic(q, b)
    on, _ = _gpu(qn, solver, obj, x0, lb, ub, PC.WINDOW, reuse=1)
    off, _ = _gpu(qn, solver, obj, x0, lb, ub, PC.WINDOW, reuse=0)
    assert on.trace()[1].tobytes() == off.trace()[1].tobytes() and on.x().tobytes() == off.x().tobytes()
    iters = len(on.trace()[0])
    assert iters >= 1 and on.newton_factorisations() == 1 and off.newton_factorisations() == iters
    host, _ = _gpu(qn, solver, RP.quadratic_fn(q, b), x0, lb, ub, PC.WINDOW)
    assert host.newton_factorisations() == len(host.trace()[0]) == iters


def test_indefinite_hessian_is_abnormal_termination(qn):
    n = 64
    d = np.ones(n)
    d[17] = -2.0
    x0 = np.full(n, 0.25)
    s = qn.ProjectedNewton(1e-8, x0, np.full(n, -1.0), np.full(n, 1.0))
    with pytest.raises(qn.AbnormalTermination, match="Cholesky"):
        s.minimize(qn.GLLQuadratic(1e-4, 10), qn.Quadratic(np.diag(d), np.zeros(n)), 10, 10)
    assert np.array_equal(s.x(), x0) and s.k() == 0
    h2 = np.array([[1.0, 0.0], [0.0, -1.0]])  # n = 2: the one-thread kernel
    fn = lambda x: (0.5 * (x[0] ** 2 - x[1] ** 2), np.array([x[0], -x[1]]), h2)  # noqa: E731
    s2 = qn.SpectralProjectedNewton(1e-8, [0.5, 0.5], fn, [-1.0, -1.0], [1.0, 1.0])
    with pytest.raises(qn.AbnormalTermination, match="Cholesky"):
        s2.minimize(qn.GLLQuadratic(1e-4, 10), fn, 10, 10)
    assert np.array_equal(s2.x(), [0.5, 0.5])


@pytest.mark.parametrize("solver", PC.SOLVERS)
def test_cholesky_failure_after_some_iterations_keeps_the_run_record(qn, solver):
    """A Hessian that stops being positive definite in iteration 3: x stays at x_2, and k, the counters, the path and s_norm / y_norm are
    those of the two iterations this call made."""
    a, c, mu, x0, _, _ = S.lse_problem()
    n = x0.size
    lb, ub = S.bounds(n, float("inf"))
    good = PC.lse_hess_fn(a, c, mu)
    two, status = _gpu(qn, solver, good, x0, lb, ub, 2)
    assert status == "max_iter" and two.k() == 2
    # the third loop-top point is x_2: hand out an indefinite Hessian there and nowhere else
    x2 = two.x()

    def bad(x):
        f, g, h = good(x)
        if np.array_equal(x, x2):
            h = h.copy()
            h[5, 5] = -1.0
        return f, g, h

    s = qn.SpectralProjectedNewton(PC.TOL, x0, bad, lb, ub) if solver == "spn" else qn.ProjectedNewton(PC.TOL, x0, lb, ub)
    s.set_trace(10, with_x=True)
    ls = qn.GLLQuadratic(1e-4, 10)
    with pytest.raises(qn.AbnormalTermination, match="Cholesky"):
        s.minimize(ls, bad, 10, 50)
    assert s.k() == 2 and s.x().tobytes() == x2.tobytes()
    st = s.stats()
    assert st["iterations"] == 2 and st["total_iterations"] == 2 and st["path"] & PATH_PNEWTON
    assert s.newton_factorisations() == 3
    if solver == "pn":
        assert s.s_norm() == two.s_norm() and s.y_norm() == two.y_norm() and s.s_norm() is not None


def test_rejections(qn):
    from test_gpu_device_closure import _Chain
    A = qn._abi
    lb, ub = np.full(2, -1.0), np.full(2, 1.0)
    fn = _two_var(10.0)
    s = qn.ProjectedNewton(1e-8, [0.5, 0.5], lb, ub)
    with pytest.raises(qn.ErrorInputParams, match="More-Thuente"):
        s.minimize(qn.MoreThuente(), fn, 5, 5)
    with pytest.raises(qn.ErrorInputParams):
        s.minimize(qn.MoreThuenteB(2), fn, 5, 5)
    with pytest.raises(qn.ErrorInputParams, match="Hessian not available in the oracle"):  # a Python closure without a Hessian
        s.minimize(qn.GLLQuadratic(1e-4, 10), lambda x: (x @ x, 2 * x), 5, 5)
    # a host oracle without host_hessian_fn, at the ABI
    cfn = A.HOST_ORACLE_FN(lambda _u, xp, nn, fp, gp: 0)
    o = A.OracleStruct()
    o.kind, o.host_fn = A.ORACLE_HOST, C.cast(cfn, C.c_void_p)
    ls = qn.GLLQuadratic(1e-4, 10)
    assert A.lib().qn_minimize(s.h, C.byref(ls.s), C.byref(o), 5, 5, None, None) == A.ERROR_INPUT_PARAMS
    assert b"Hessian not available" in A.lib().qn_last_error_message()
    # a log-sum-exp objective and a device closure have no Hessian here
    a, c, mu, x0, lo, hi = S.lse_problem()
    for cls, args in ((qn.ProjectedNewton, ()), ):
        p = cls(1e-8, x0, *args, lo, hi)
        with pytest.raises(qn.ErrorInputParams, match="Hessian not available"):
            p.minimize(ls, qn.LogSumExp(a, c, mu), 5, 5)
    ca, cc, cx0, clb, cub = S.chain_problem(n=64)
    ch = _Chain(qn, ca, cc)
    try:
        p = qn.ProjectedNewton(1e-8, cx0, clb, cub)
        with pytest.raises(qn.ErrorInputParams, match="Hessian not available"):
            p.minimize(ls, ch.closure, 5, 5)
        with pytest.raises(qn.ErrorInputParams, match="Hessian not available"):
            qn.SpectralProjectedNewton(1e-8, cx0, ch.closure, clb, cub)
    finally:
        ch.close()
    with pytest.raises(qn.ErrorInputParams):
        s.compute_direction((0.0, np.ones(2)))
    with pytest.raises(qn.ErrorInputParams):  # lambda belongs to the spectral solvers
        qn.solver._check(A.lib().qn_solver_set_spg_lambdas(s.h, 1e-2, 1e2))
    sp = qn.SpectralProjectedNewton(1e-8, [0.5, 0.5], fn, lb, ub).with_lambdas(1e-2, 1e2)
    assert (sp.lambda_min(), sp.lambda_max()) == (1e-2, 1e2) and sp.lambda_() == 1.0 / 1.5  # 1 / ||P(x0 - g0) - x0||_inf with d0 = (-0.5, -1.5); with_lambdas does not clamp it again
    v = C.c_size_t(7)
    b = qn.BFGS(1e-8, [0.5, 0.5])
    assert A.lib().qn_solver_newton_factorisations(b.h, C.byref(v)) == A.OK and v.value == 0


def test_world_above_one_is_rejected(qn):
    from thread_ranks import run_ranks

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        seen = []
        eye = np.eye(32)
        for cls, args in ((qn.ProjectedNewton, ()), (qn.SpectralProjectedNewton, (lambda x: (0.0, x, eye),))):
            with pytest.raises(qn.ErrorInputParams, match="one rank"):
                cls(1e-6, np.zeros(32), *args, -np.ones(32), np.ones(32), ctx=ctx)
            seen.append(cls.__name__)
        ctx.close()
        return seen
    assert run_ranks(2, body, timeout=60.0) == [["ProjectedNewton", "SpectralProjectedNewton"]] * 2


def test_non_symmetric_hessian_lower_triangle(qn, qo):
    """Only the lower triangle is read, as nalgebra's Cholesky does: junk above the diagonal changes nothing (and takes no LU path)."""
    n = 64
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, 0.05)
    junk = np.tril(q) + np.triu(np.full((n, n), 123.0), 1)
    base = R.quadratic_fn(q, b)
    fn = lambda x: (*base(x), junk)  # noqa: E731
    lip = float(np.max(np.sum(np.abs(q), axis=1)))
    s, ref, _ = _check_case(qn, "spn", fn, fn, x0, lb, ub, lip)
    clean, _, _ = PC.run_ref("spn", RP.quadratic_fn(q, b), x0, lb, ub, PC.WINDOW)
    assert np.array(ref.trace_x).tobytes() == np.array(clean.trace_x).tobytes()


@pytest.mark.parametrize("solver", PC.SOLVERS)
def test_warm_restart_reset_and_callback(qn, solver):
    a, c, mu, x0, _, _ = S.lse_problem()
    lb, ub = S.bounds(x0.size, float("inf"))
    fn = PC.lse_hess_fn(a, c, mu)
    ks = []
    one, _ = _gpu(qn, solver, fn, x0, lb, ub, 12, callback=lambda s: ks.append(s.k()))
    assert ks == list(range(1, 13))  # the callback sees k after k += 1 (ls_solver.rs:104-107)
    two = qn.SpectralProjectedNewton(PC.TOL, x0, fn, lb, ub) if solver == "spn" else qn.ProjectedNewton(PC.TOL, x0, lb, ub)
    ls = qn.GLLQuadratic(1e-4, 10)
    for _ in range(2):
        with pytest.raises(qn.MaxIterReached):
            two.minimize(ls, fn, 6, 50)
        assert two.k() == 6
    assert one.x().tobytes() == two.x().tobytes()
    if solver == "spn":
        assert one.lambda_() == two.lambda_()
        two.reset(x0)
        assert two.lambda_() is None
    else:
        assert one.s_norm() == two.s_norm() and one.y_norm() == two.y_norm() and two.s_norm() is not None
        two.reset(x0)
        assert two.s_norm() is None and two.y_norm() is None and not two.next_iterate_too_close()
    assert np.array_equal(two.x(), x0)


def test_warm_restart_device_quadratic_keeps_the_factor(qn, qo):
    n = 512
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, 0.05)
    obj = qn.Quadratic(q, b)
    one, _ = _gpu(qn, "spn", obj, x0, lb, ub, 30)
    two = qn.SpectralProjectedNewton(PC.TOL, x0, obj, lb, ub)
    ls = qn.GLLQuadratic(1e-4, 10)
    counts = []
    for _ in range(2):
        with pytest.raises(qn.MaxIterReached):
            two.minimize(ls, obj, 15, 50)
        counts.append(two.newton_factorisations())
    assert counts == [1, 0]
    assert one.x().tobytes() == two.x().tobytes() and one.lambda_() == two.lambda_()


def test_converged_run_enqueues_no_factorisation(qn, qo):
    """The loop top is decided before the factorisation is enqueued: a start that already satisfies the test, and a cap of 0, cost none."""
    n = 512
    q, b, _, _ = S.problem(qo, n)
    xs = np.linalg.solve(q, b)
    obj = qn.Quadratic(q, b)
    s = qn.ProjectedNewton(1e-3, xs, np.full(n, -np.inf), np.full(n, np.inf))
    s.minimize(qn.GLLQuadratic(1e-4, 10), obj, 10, 10)
    assert s.k() == 0 and s.newton_factorisations() == 0
    sp = qn.SpectralProjectedNewton(1e-10, np.zeros(n), obj, np.full(n, -1.0), np.full(n, 1.0))
    assert sp.newton_factorisations() == 0 and sp.lambda_() is not None
    # a memoised run that converges: one factorisation per iteration that computed a direction, none for the loop top that ended it
    pn, status = _gpu(qn, "pn", obj, np.zeros(n), np.full(n, -np.inf), np.full(n, np.inf), 10, reuse=0)
    assert status == "ok" and pn.newton_factorisations() == pn.k() >= 1


def test_work_matrix_is_allocated_by_the_first_direction(qn):
    """The n x n work matrix belongs to the first iteration that computes a direction: a converged start, a cap of 0 and SpectralProjectedNewton's
    constructor call leave the solver with its O(n) state."""
    import torch
    n = PC.BIG_N
    diag = P.synth_diag(n, S.KAPPA)
    b, x0 = P.synth_vectors(n, P.SEED)
    lb, ub = S.bounds(n, 0.05)
    obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
    ls = qn.GLLQuadratic(1e-4, 10)
    warm = qn.SpectralProjectedGradient(PC.TOL, x0, obj, lb, ub)  # whatever a first evaluation allocates lazily stays outside the measurement
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    pn = qn.ProjectedNewton(1e30, x0, lb, ub)
    pn.minimize(ls, obj, 10, 10)  # converged at the first loop top
    capped = qn.ProjectedNewton(PC.TOL, x0, lb, ub)
    with pytest.raises(qn.MaxIterReached):
        capped.minimize(ls, obj, 0, 10)
    spn = qn.SpectralProjectedNewton(PC.TOL, x0, obj, lb, ub)  # lambda0: the constructor's batch
    assert pn.k() == 0 and capped.k() == 0 and spn.lambda_() is not None
    free1, _ = torch.cuda.mem_get_info()
    # three solvers of at most 24 n doubles each (test_gpu_spg.test_memory_is_linear_in_n) and 32 MiB for the allocator's granularity over
    # their small buffers; one n x n matrix alone would be 128 MiB
    assert free0 - free1 <= 3 * 24 * n * 8 + (32 << 20), (free0 - free1) / (1 << 20)
    with pytest.raises(qn.MaxIterReached):
        spn.minimize(ls, obj, 1, 10)
    free2, _ = torch.cuda.mem_get_info()
    assert free1 - free2 >= n * n * 8, (free1 - free2) / (1 << 20)  # the measurement sees the matrix when it is made
    warm.close()


def test_pnewton_example_cpp():
    """examples/pnewton_example.cpp: both solvers through the C++ mirror (include/qn_solver.hpp), closures carrying their Hessian."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pnewton_example.bin")
    assert os.path.exists(exe), "examples/pnewton_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("pnewton example ok")
