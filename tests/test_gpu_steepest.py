"""GPU tests of QN_PNORM_DESCENT, QN_COORDINATE_DESCENT and QN_LS_NO_SEARCH (steepest_descent/pnorm_descent.rs, coordinate_descent.rs,
line_search/nosearch.rs) against the restatement tests/ref_steepest.py on the problems of tests/steepest_cases.py.

Sizes of the p-norm direction kernel (csrc/qn_pnorm.hip.h): n = 2 (the control kernel's literal column sweep, decision for decision), 7 (under one
wave's width of 16-byte lanes), 130 (ragged rows and columns, n_pad = 144: padding must stay out of the sums), 1030 (more than one workgroup's
rows), 4100 (just above the kernel's LDS column chunk, QN_PN_CH = 4096 columns of g per chunk: the second chunk holds the last 16 columns).

Tolerances.  Iterate sequences: tests/steepest_cases.py (the window's recorded CPU order spread x 8, floor 16 ulp, relative to the compared array's
largest magnitude -- fixed before any GPU run).  The direction kernel alone: the element-wise a-priori bound written out at `_direction_bound`."""
import math
import os
import subprocess

import numpy as np
import pytest

import ref_steepest as R
import spg_cases
import steepest_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS53 = 2.0 ** -53
KERNEL_SIZES = [7, 130, 1030, 4100]


def _line_search(qn, ls):
    return {"mt": qn.MoreThuente, "bt": lambda: qn.BackTracking(1e-4, 0.5), "none": qn.NoSearch}[ls]()


class _Oracle:
    """the window's problem as the oracle kind it is meant to exercise; close() releases what it holds"""

    def __init__(self, qn, kind, pr):
        self.chain = None
        if kind in ("two_var", "quad_host"):
            self.oracle = pr["fn"]
        elif kind == "quad_dev":
            self.oracle = qn.Quadratic(*pr["data"])
        elif kind == "lse":
            self.oracle = qn.LogSumExp(*pr["data"])
        else:
            from test_gpu_device_closure import _Chain
            self.chain = _Chain(qn, *pr["data"])
            self.oracle = self.chain.closure

    def close(self):
        if self.chain:
            self.chain.close()


def _run(qn, s, ls, oracle, iters, memoize, max_ls=SC.MAX_LS, callback=None):
    s.memoize = memoize
    s.set_trace(max(iters, 1), with_x=True)
    status = "ok"
    try:
        s.minimize(_line_search(qn, ls), oracle, iters, max_ls, callback=callback)
    except qn.MaxIterReached:
        status = "max_iter"
    return status


def _close(name, got, want, tol):
    d = SC.rel_diff(got, want)
    print(f"    {name}: rel diff {d:.3e} (tolerance {tol:.3e})")
    return d <= tol


def _rand_p(n, seed=0):
    rng = np.random.default_rng(500 + n + seed)
    return rng.standard_normal((n, n)) / math.sqrt(n), rng.standard_normal(n)  # any matrix: neither symmetric nor definite


# ---- fails without the feature ----
def test_create_succeeds(qn):
    s = qn.PnormDescent(1e-8, np.zeros(7), np.eye(7))
    c = qn.CoordinateDescent(1e-8, np.zeros(7))
    assert s.k() == 0 and c.k() == 0 and s.grad_tol() == 1e-8
    s.close()
    c.close()


# ---- the reference's own tests, n = 2: decision for decision ----
@pytest.mark.parametrize("memoize", [0, 1])
@pytest.mark.parametrize("name,solver,ls,iters,calls", SC.REFERENCE_TESTS)
def test_reference_tests_on_the_gpu(qn, name, solver, ls, iters, calls, memoize):
    """minimize(.., 1000, 100): x, k, t per iteration and the oracle-call counts equal the restatement's exactly; |f| < 1e-6 as the reference asserts"""
    fn = SC.two_var()
    ref, o, status = SC.run_ref(solver, fn, SC.X0_2D.copy(), ls, 1000, SC.INVERSE_P_2D, max_ls=100)
    s = qn.PnormDescent(SC.TOL, SC.X0_2D, SC.INVERSE_P_2D) if solver == "pnorm" else qn.CoordinateDescent(SC.TOL, SC.X0_2D)
    assert _run(qn, s, ls, fn, 1000, memoize, max_ls=100) == status == "ok"
    tr, xs = s.trace()
    st = s.stats()
    f, g = fn(s.x())
    assert abs(f - 0.0) < 1e-6 and s.has_converged((f, g))
    assert s.k() == ref.k == iters and st["oracle_calls"] == o.calls == calls
    assert st["oracle_evals"] == (o.evals if memoize else o.calls)
    assert [r["t"] for r in tr] == [r["t"] for r in ref.trace]
    assert [r["n_evals"] for r in tr] == [r["n_evals"] for r in ref.trace]
    assert np.array_equal(xs, np.array(ref.trace_x)) and np.array_equal(s.x(), ref.x)
    assert [r["gnorm"] for r in tr] == [r["gnorm"] for r in ref.trace]
    assert not st["path"] & (qn._abi.PATH_PNORM | qn._abi.PATH_PIPELINED)  # n <= 5: the control kernel alone
    s.close()


# ---- PnormDescent: iterate-sequence parity beyond n = 5 ----
@pytest.mark.parametrize("memoize", [0, 1])
@pytest.mark.parametrize("name", list(SC.WINDOWS))
def test_window_parity(qn, qo, name, memoize):
    w = SC.WINDOWS[name]
    pr, ref, o, _ = SC.window_ref(name, qo)
    orc = _Oracle(qn, w["problem"], pr)
    try:
        s = qn.PnormDescent(SC.TOL, pr["x0"], pr["p"])
        status = _run(qn, s, w["ls"], orc.oracle, w["K"], memoize)
        tr, xs = s.trace()
        st = s.stats()
        tol = SC.tolerance(w)
        print(f"{name} memoize={memoize}: k={s.k()} calls={st['oracle_calls']}/{o.calls} evals={st['oracle_evals']}/{o.evals} path={st['path']}")
        assert status == "max_iter" and s.k() == w["K"] == len(tr)
        ok = _close("x-trace", xs, np.array(ref.trace_x), tol)
        ok &= _close("f", [r["f"] for r in tr], [r["f"] for r in ref.trace], tol)
        ok &= _close("gnorm", [r["gnorm"] for r in tr], [r["gnorm"] for r in ref.trace], tol)
        ok &= _close("t", [r["t"] for r in tr], [r["t"] for r in ref.trace], tol)
        assert ok
        assert [r["n_evals"] for r in tr] == [r["n_evals"] for r in ref.trace]
        assert st["oracle_calls"] == o.calls
        assert st["oracle_evals"] == (o.evals if memoize else o.calls)
        if orc.chain and not memoize:
            assert orc.chain.calls() == o.calls
        n_pad = (w["n"] + 15) // 16 * 16
        assert st["path"] & qn._abi.PATH_PNORM
        assert not st["path"] & (qn._abi.PATH_FUSED | qn._abi.PATH_SYM | qn._abi.PATH_SYM_GENERIC | qn._abi.PATH_SYM2 | qn._abi.PATH_PIPELINED | qn._abi.PATH_RANK1)
        assert st["h_passes"] == w["K"] and st["h_bytes"] == w["K"] * n_pad * n_pad * 8  # ONE read-only stream of inverse_p per iteration
        assert np.array_equal(s.inverse_p(), pr["p"])  # ... which no kernel writes
        s.close()
    finally:
        orc.close()


# ---- the direction kernel alone, through compute_direction ----
def _direction_bound(p, g):
    """|d_i - exact_i| <= (n + 2) 2^-53 sum_j |P_ij| |g_j|: a sum of n products in ANY order, with or without fused multiply-adds, carries at most
    (n - 1) roundings of partial sums and n of products, each relative 2^-53 to a quantity bounded by the sum of the magnitudes; the negation is exact"""
    return (p.shape[0] + 2) * EPS53 * (np.abs(p) @ np.abs(g))


def _exact_direction(p, g):
    return -np.array([math.fsum((row * g).tolist()) for row in p])


@pytest.mark.parametrize("n", KERNEL_SIZES)
def test_direction_kernel(qn, n):
    p, g = _rand_p(n)
    p[n // 2, :] = 0.0  # a row of zeros
    s = qn.PnormDescent(1e-12, np.zeros(n), p)
    d = s.compute_direction((0.0, g))
    exact, bound = _exact_direction(p, g), _direction_bound(p, g)
    ratio = float(np.max(np.abs(d - exact)[bound > 0] / bound[bound > 0]))
    print(f"n = {n}: max |d - exact| / bound = {ratio:.3e}")
    assert np.all(np.abs(d - exact) <= bound)
    assert np.max(np.abs(d + p.T @ g)) > 1e6 * np.max(bound)  # rows of inverse_p, not columns: the case discriminates
    assert d[n // 2] == 0.0 and R.PnormDescent(1e-12, np.zeros(n), p).compute_direction((0.0, g))[n // 2] == 0.0  # exactly zero (either sign), as the restatement's
    assert s.compute_direction((0.0, g)).tobytes() == d.tobytes()  # two calls: identical bits
    assert s.stats()["path"] & qn._abi.PATH_PNORM
    # every instance of the kernel -- rows per wave 2 / 4, plain / non-temporal loads -- gives the same bits
    for rw, nt in ((2, 0), (2, 1), (4, 0), (4, 1)):
        s.set_option("pnorm_rows_per_wave", rw)
        s.set_option("pnorm_nontemporal", nt)
        assert s.compute_direction((0.0, g)).tobytes() == d.tobytes(), (rw, nt)
    s.close()


def test_direction_literal_order_at_small_n(qn):
    p, g = _rand_p(5)
    s = qn.PnormDescent(1e-12, np.zeros(5), p)
    want = R.PnormDescent(1e-12, np.zeros(5), p).compute_direction((0.0, g))  # y = P[:,0] g_0; y += P[:,j] g_j
    assert np.array_equal(s.compute_direction((0.0, g)), want)
    s.close()


def test_direction_kernel_keeps_the_padding_out(qn):
    """n = 130 (n_pad = 144): NaN / inf in the gradient's LOGICAL entries reach d as IEEE says; nothing else does"""
    n = 130
    p, g = _rand_p(n, seed=1)
    p[3, :] = 0.0
    p[:, n - 1] = 0.0
    p[7, n - 1] = 1.0
    g[n - 1] = float("inf")  # the last logical column: only row 7 multiplies it by something else than 0 -- and 0 * inf = NaN in every other row
    s = qn.PnormDescent(1e-12, np.zeros(n), p)
    d = s.compute_direction((0.0, g))
    assert d[7] == -float("inf") and np.all(np.isnan(np.delete(d, 7)))
    s.close()


# ---- CoordinateDescent ----
def test_coordinate_descent_sign_quirk(qn):
    """the runs of tests/test_ref_steepest.py::test_coordinate_descent_sign_quirk: -e_1, then -e_0 on a NEGATIVE gradient entry -- an ascent
    direction -- with the steps and iterates of the restatement, exactly"""
    for x0, iters, tol in ((np.array([-3.0, 1.0]), 3, SC.TOL), (np.array([-(0.5 ** 60), 1.0]), 2, 1e-30)):
        ref, o, _ = SC.run_ref("cd", SC.two_var(), x0, "bt", iters, tol=tol, max_ls=100)
        s = qn.CoordinateDescent(tol, x0)
        assert _run(qn, s, "bt", SC.two_var(), iters, 0, max_ls=100) == "max_iter"
        tr, xs = s.trace()
        assert [r["t"] for r in tr] == [r["t"] for r in ref.trace]
        assert np.array_equal(xs, np.array(ref.trace_x))
        assert s.stats()["oracle_calls"] == o.calls
        s.close()
    assert [r["t"] for r in ref.trace] == [1.0, 0.5 ** 100]  # (the second run exhausts max_iter_line_search = 100)


def test_coordinate_descent_directions(qn):
    nan = float("nan")
    n = 2 ** 18 + 3
    s = qn.CoordinateDescent(1e-12, np.zeros(n))
    e0 = np.zeros(n)
    e0[0] = -1.0
    assert np.array_equal(s.compute_direction((0.0, np.zeros(n))), e0)          # the all-zero gradient: -e_0
    assert np.array_equal(s.compute_direction((0.0, np.full(n, nan))), e0)      # all NaN: nothing ever wins
    g = np.zeros(n)
    g[[5000, 200000, n - 1]] = [-6.0, 6.0, -6.0]  # equal largest magnitudes in three workgroups' ranges (2048 indices each), the last in the ragged tail
    g[[4000, 100000]] = nan                       # ... and NaN entries in front of and between them
    d = s.compute_direction((0.0, g))
    assert d[5000] == -1.0 and np.count_nonzero(d) == 1  # the smallest index wins; -1.0 although g_p < 0
    g[n - 1] = -6.5
    d = s.compute_direction((0.0, g))
    assert d[n - 1] == -1.0 and np.count_nonzero(d) == 1
    s.close()
    for m in (2, 7, 130, 2049):
        c = qn.CoordinateDescent(1e-12, np.zeros(m))
        rng = np.random.default_rng(m)
        gm = rng.standard_normal(m)
        gm[m // 2] = gm[m - 1] = -np.max(np.abs(gm)) - 1.0
        want = R.CoordinateDescent(1e-12, np.zeros(m)).compute_direction((0.0, gm))
        assert np.array_equal(c.compute_direction((0.0, gm)), want)
        c.close()


def test_coordinate_descent_ties_across_workgroups_device_closure(qn):
    """n = 2^18 + 3 through examples/device_closure.hip (the chain with c = 0: g_i = x_i (x_i^2 - a_i), separable): x0 has the same entry at three
    indices in different workgroups' ranges, so |g| has three equal largest magnitudes; one iteration moves the SMALLEST of those indices only"""
    from test_gpu_device_closure import _Chain
    n = 2 ** 18 + 3
    a = np.ones(n)
    x0 = np.zeros(n)
    x0[[5000, 200000, n - 1]] = 2.0  # g = 2 (4 - 1) = 6 at each
    chain = _Chain(qn, a, 0.0)
    try:
        fn = spg_cases.chain_fn(a, 0.0)
        ref, o, _ = SC.run_ref("cd", fn, x0, "bt", 1)
        s = qn.CoordinateDescent(1e-12, x0)
        assert _run(qn, s, "bt", chain.closure, 1, 0) == "max_iter"
        tr, xs = s.trace()
        moved = np.flatnonzero(xs[0] != x0)
        assert moved.tolist() == [5000] and xs[0][5000] == x0[5000] - tr[0]["t"]
        assert tr[0]["t"] == ref.trace[0]["t"] and np.array_equal(xs[0], ref.trace_x[0])
        assert tr[0]["gnorm"] == 6.0
        s.close()
    finally:
        chain.close()


def test_coordinate_descent_nan_gradient_entries(qn):
    """f finite, NaN entries in g: they never win the fold and are ignored by ||g||_inf, but g.d -- a full dot product in the reference -- is NaN, so
    BackTracking never accepts and returns beta^max_iter; the restatement does the same"""
    nan = float("nan")

    def fn(x):
        g = x.copy()
        g[[2, 5]] = nan
        return 0.5 * float(x @ x), g
    x0 = np.array([1.0, -4.0, 9.0, 4.0, 0.5, -7.0, 2.0])
    ref, o, _ = SC.run_ref("cd", fn, x0, "bt", 2, max_ls=5)
    s = qn.CoordinateDescent(1e-12, x0)
    assert _run(qn, s, "bt", fn, 2, 0, max_ls=5) == "max_iter"
    tr, xs = s.trace()
    assert [r["t"] for r in tr] == [r["t"] for r in ref.trace] == [0.5 ** 5] * 2
    assert np.array_equal(xs, np.array(ref.trace_x)) and [r["gnorm"] for r in tr] == [r["gnorm"] for r in ref.trace] == [4.0, 4.03125]
    assert s.stats()["oracle_calls"] == o.calls
    s.close()


# ---- NoSearch ----
def test_nosearch_gradient_descent_and_pnorm(qn, qo):
    w = SC.WINDOWS["p7_mt"]
    pr, _, _, _ = SC.window_ref("p7_mt", qo)
    K = 3
    ref, o, _ = SC.run_ref("gd", pr["fn"], pr["x0"], "none", K)
    s = qn.GradientDescent(SC.TOL, pr["x0"])
    assert _run(qn, s, "none", pr["fn"], K, 0) == "max_iter"
    tr, xs = s.trace()
    assert np.array_equal(xs, np.array(ref.trace_x)) and [r["t"] for r in tr] == [1.0] * K  # x + d with d = -g: exact
    assert s.stats()["oracle_calls"] == o.calls == K  # one call per iteration: the line search makes none
    s.close()
    ref, o, _ = SC.run_ref("pnorm", pr["fn"], pr["x0"], "none", K, pr["p"])
    s = qn.PnormDescent(SC.TOL, pr["x0"], pr["p"])
    assert _run(qn, s, "none", pr["fn"], K, 0) == "max_iter"
    tr, xs = s.trace()
    assert _close("x-trace", xs, np.array(ref.trace_x), SC.tolerance(SC.NOSEARCH_WINDOW)) and [r["t"] for r in tr] == [1.0] * K
    assert s.stats()["oracle_calls"] == o.calls == K and [r["ls_iters"] for r in tr] == [0] * K
    s.close()
    assert qn.NoSearch().compute_step_len(pr["x0"], pr["fn"](pr["x0"]), -pr["fn"](pr["x0"])[1], pr["fn"], 10) == 1.0  # LineSearch::compute_step_len on its own
    assert w["n"] == 7


def test_nosearch_newton_is_the_pure_newton_step(qn, qo):
    """an SPD quadratic at n = 130: one iteration of x + d reaches the minimiser (the bound tests/test_gpu_newton.py puts on a Newton step)"""
    pr, _, _, _ = SC.window_ref("p130_bt", qo)
    q, b = pr["data"]
    s = qn.Newton(1e-10, pr["x0"])
    s.set_trace(1, with_x=True)
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.NoSearch(), qn.Quadratic(q, b), 1, 20)
    tr, xs = s.trace()
    xstar = np.linalg.solve(q, b)
    assert tr[0]["t"] == 1.0 and tr[0]["ls_iters"] == 0
    assert np.linalg.norm(xs[0] - xstar) <= 1e-9 * np.linalg.norm(xstar)
    s.close()


def test_nosearch_is_rejected_where_it_is_not_built(qn):
    fn = lambda x: (0.5 * float(x @ x), x)  # noqa: E731
    for make in (lambda: qn.BFGS(1e-8, np.ones(7)), lambda: qn.SpectralProjectedGradient(1e-8, np.ones(7), fn, np.full(7, -2.0), np.full(7, 2.0))):
        s = make()
        with pytest.raises(qn.ErrorInputParams):
            s.minimize(qn.NoSearch(), fn, 5, 5)
        s.close()


# ---- errors and plumbing ----
def test_minimize_without_inverse_p_and_setter_on_other_methods(qn):
    A = qn._abi
    s = qn.GradientDescent(1e-8, np.ones(7))
    bare = qn.PnormDescent(1e-8, np.ones(7), None)  # qn_solver_create alone: the matrix has not been set
    with pytest.raises(qn.ErrorInputParams, match="inverse_p"):
        bare.minimize(qn.MoreThuente(), lambda x: (0.5 * float(x @ x), x), 5, 5)
    with pytest.raises(qn.ErrorInputParams, match="inverse_p"):
        bare.inverse_p()
    with pytest.raises(qn.ErrorInputParams, match="inverse_p"):
        bare.compute_direction((0.0, np.ones(7)))
    bare.set_inverse_p(2.0 * np.eye(7))
    assert np.array_equal(bare.compute_direction((0.0, np.ones(7))), np.full(7, -2.0))
    bare.close()
    b = qn.BFGS(1e-8, np.ones(7))
    eye = np.eye(7)
    assert A.lib().qn_solver_set_inverse_p(b.h, eye.ctypes.data_as(A.dp)) == A.ERROR_INPUT_PARAMS
    assert A.lib().qn_solver_get_inverse_p(b.h, eye.ctypes.data_as(A.dp)) == A.ERROR_INPUT_PARAMS
    assert A.lib().qn_solver_set_inverse_p(s.h, eye.ctypes.data_as(A.dp)) == A.ERROR_INPUT_PARAMS
    b.close()
    s.close()


def test_world_above_one_is_rejected(qn):
    """ranks as threads, as tests/test_gpu_partitions.py"""
    from thread_ranks import run_ranks

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        with pytest.raises(qn.ErrorInputParams, match="one rank"):
            qn.PnormDescent(1e-6, np.zeros(32), np.eye(32), ctx=ctx)
        with pytest.raises(qn.ErrorInputParams, match="one rank"):
            qn.CoordinateDescent(1e-6, np.zeros(32), ctx=ctx)
        ctx.close()
        return True
    assert run_ranks(2, body, timeout=60.0) == [True, True]


def test_inverse_p_round_trip_reset_and_warm_restart(qn, qo):
    w = SC.WINDOWS["p130_bt"]
    pr, ref, _, _ = SC.window_ref("p130_bt", qo)
    obj = qn.Quadratic(*pr["data"])
    K = w["K"]
    one = qn.PnormDescent(SC.TOL, pr["x0"], pr["p"])
    assert one.inverse_p().tobytes() == np.ascontiguousarray(pr["p"]).tobytes()  # bit-equal, any matrix
    assert _run(qn, one, w["ls"], obj, K, 0) == "max_iter"
    two = qn.PnormDescent(SC.TOL, pr["x0"], pr["p"])
    for _ in range(2):  # a warm restart continues the sequence
        assert _run(qn, two, w["ls"], obj, K // 2, 0) == "max_iter" and two.k() == K // 2
    assert one.x().tobytes() == two.x().tobytes()
    two.reset(pr["x0"])  # inverse_p is a constructor argument, not state: reset keeps it
    assert two.k() == 0 and np.array_equal(two.x(), pr["x0"]) and np.array_equal(two.inverse_p(), pr["p"])
    assert _run(qn, two, w["ls"], obj, K, 0) == "max_iter"
    assert one.x().tobytes() == two.x().tobytes()
    one.close()
    two.close()


def test_callback_sees_every_iteration(qn, qo):
    w = SC.WINDOWS["p130_bt"]
    pr, ref, _, _ = SC.window_ref("p130_bt", qo)
    seen = []
    s = qn.PnormDescent(SC.TOL, pr["x0"], pr["p"])
    assert _run(qn, s, w["ls"], qn.Quadratic(*pr["data"]), w["K"], 1, callback=lambda me: seen.append((me.k(), me.x()))) == "max_iter"
    assert [k for k, _ in seen] == list(range(1, w["K"] + 1))
    assert SC.rel_diff(np.array([x for _, x in seen]), np.array(ref.trace_x)) <= SC.tolerance(w)
    s.close()
    seen = []
    c = qn.CoordinateDescent(SC.TOL, SC.X0_2D)
    ref, _, _ = SC.run_ref("cd", SC.two_var(), SC.X0_2D.copy(), "mt", 4)
    assert _run(qn, c, "mt", SC.two_var(), 4, 0, callback=lambda me: seen.append((me.k(), me.x()))) == "max_iter"
    assert [k for k, _ in seen] == [1, 2, 3, 4] and np.array_equal(np.array([x for _, x in seen]), np.array(ref.trace_x))
    c.close()
