"""GPU tests of QN_BROYDEN (Broyden / BroydenB, quasi_newton/broyden.rs, broyden_b.rs) against the restatement tests/ref_broyden.py on the windows
of tests/broyden_cases.py.  Sizes: n = 2 (the one-workgroup path in the reference's literal order), 7 (one ragged tile of csrc/qn_rank1.hip.h), 130
(2 x 2 tiles, ragged edge: padding must stay zero), 384 (3 x 3 tiles: the second stage sums three row blocks), 1024 (8 x 8).

Tolerances.  Iterate sequences: tests/broyden_cases.py (the window's recorded CPU order spread x 8, floor 16 ulp, relative to the compared array's
largest magnitude -- fixed before any GPU run).  The single-update unit test: an element-wise a-priori bound, written out at `_update_bound`, at the
tile edges (n = 128, 129, 257 too) and on a matrix over twelve decades.  Whole runs entry by entry: tests/test_gpu_broyden_replay.py."""
import os
import subprocess

import numpy as np
import pytest

import broyden_cases as BC
import ref_broyden as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _line_search(qn, ls, lb, ub, n):
    if ls == "mt":
        return qn.MoreThuente()
    if ls == "bt":
        return qn.BackTracking(1e-4, 0.5)
    if lb is None:
        lb, ub = np.full(n, -np.inf), np.full(n, np.inf)
    if ls == "mtb":
        return qn.MoreThuenteB(n).with_lower_bound(lb).with_upper_bound(ub)
    return qn.BackTrackingB(1e-4, 0.5, lb, ub)


class _Oracle:
    """the window's problem as the oracle kind it is meant to exercise; close() releases what it holds"""

    def __init__(self, qn, w, pr):
        self.chain = None
        kind = w["problem"]
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


def _solver(qn, pr, tol=BC.TOL):
    if pr["lb"] is None:
        return qn.Broyden(tol, pr["x0"])
    return qn.BroydenB(tol, pr["x0"], pr["lb"], pr["ub"])


def _run(qn, w, pr, oracle, iters, memoize, s=None):
    s = s or _solver(qn, pr)
    s.memoize = memoize
    s.set_trace(max(iters, 1), with_x=True)
    status = "ok"
    try:
        s.minimize(_line_search(qn, w["ls"], pr["lb"], pr["ub"], w["n"]), oracle, iters, BC.MAX_LS)
    except qn.MaxIterReached:
        status = "max_iter"
    return s, status


def _close(name, got, want, tol):
    d = BC.rel_diff(got, want)
    print(f"    {name}: rel diff {d:.3e} (tolerance {tol:.3e})")
    return d <= tol


# ---- fails without the feature ----
def test_create_succeeds(qn):
    s = qn.Broyden(1e-8, np.zeros(7))
    assert s.k() == 0 and s.s_norm() is None and s.y_norm() is None
    assert np.array_equal(s.approx_inv_hessian(), np.eye(7))
    s.close()


# ---- the kernel on its own ----
def _update_bound(h, s, y):
    """Element-wise bound on |computed - exact| of H+ = H + c a w' (a = s - H y, w = H' s, c = 1 / s.y) for ANY summation order, with or without
    fused multiply-adds: a sum of n products carries at most gamma = (n + 2) eps times the sum of their magnitudes; a, c, w and the final
    (a_i w_j) c + h_ij add a handful of roundings each (4 more gammas cover them)."""
    n = s.size
    g = (n + 6) * EPS
    A = np.abs(s) + np.abs(h) @ np.abs(y)           # |a_i| and its error are both within g A_i of ... A_i
    W = np.abs(h).T @ np.abs(s)                     # |w_j| <= W_j, error <= g W_j
    kappa = (np.abs(s) @ np.abs(y)) / abs(s @ y)    # relative error of the denominator: kappa g
    return g * np.abs(h) + (4.0 + kappa) * g / abs(s @ y) * np.outer(A, W)


SINGLE_N = [2, 7, 128, 129, 130, 257, 384]  # 128: one exactly full tile; 129: the edge tile has one live column; 257: a ragged third tile


@pytest.mark.parametrize("n", SINGLE_N)
def test_single_update_on_a_non_symmetric_h(qn, n):
    _single_update(qn, n, False)


@pytest.mark.parametrize("n", SINGLE_N)
def test_single_update_on_a_non_symmetric_h_over_twelve_decades(qn, n):
    """the second matrix: D1 M D2 with D = diag(10^U(-3, 3)), where only an element-wise bound sees the small entries.  (The seeds 200 + n were
    picked on the CPU: both discrimination margins below stand at 5e10 or more, the reference's own order at 2e-2 of the bound or less.)"""
    _single_update(qn, n, True)


def _single_update(qn, n, scaled):
    rng = np.random.default_rng((200 if scaled else 100) + n)
    h = np.eye(n) + rng.standard_normal((n, n)) / np.sqrt(n)
    if scaled:
        d1, d2 = 10.0 ** rng.uniform(-3, 3, n), 10.0 ** rng.uniform(-3, 3, n)
        h = (d1[:, None] * h) * d2[None, :]
    s, y = rng.standard_normal(n), rng.standard_normal(n)
    want = R.broyden_update(h, s, y, "factored", "fsum")
    bound = _update_bound(h, s, y)
    # the case discriminates: with w = H s (right only for a symmetric H) the result is another matrix, by far more than the bound
    a = s - h @ y
    wrong = h + np.outer(a, h @ s) / (s @ y)
    assert np.max(np.abs(wrong - want)) > 1e6 * np.max(bound)
    assert np.max(np.abs(R.broyden_update(h, s, y, "literal", "dot") - want) / bound) <= 1.0  # (the reference's own order is inside the bound too)
    b = qn.Broyden(1e-12, np.zeros(n))
    b.set_approx_inv_hessian(h)
    assert np.array_equal(b.approx_inv_hessian(), h)
    g = rng.standard_normal(n)
    d = b.compute_direction((0.0, g))
    gb = (n + 2) * EPS * (np.abs(h) @ np.abs(g))
    assert np.all(np.abs(d + h @ g) <= gb)                      # rows of H ...
    assert np.max(np.abs(d + h.T @ g)) > 1e6 * np.max(gb)       # ... not columns
    b.secant_update(s, y)
    got = b.approx_inv_hessian()
    ratio = float(np.max(np.abs(got - want) / bound))
    print(f"n = {n}{' scaled' if scaled else ''}: max |H+ - restatement| / bound = {ratio:.3e}")
    assert ratio <= 1.0
    assert b.s_norm() == pytest.approx(np.linalg.norm(s), rel=1e-14) and b.y_norm() == pytest.approx(np.linalg.norm(y), rel=1e-14)
    b.close()


def test_secant_update_hook_honours_the_skip_rule(qn):
    n = 130
    rng = np.random.default_rng(7)
    h = np.eye(n) + 0.1 * rng.standard_normal((n, n))
    b = qn.BroydenB(1e-3, np.zeros(n), -np.ones(n), np.ones(n))
    b.set_approx_inv_hessian(h)
    b.secant_update(1e-6 * rng.standard_normal(n), rng.standard_normal(n))  # ||s|| < tol: recorded, H untouched
    assert b.next_iterate_too_close() and not b.gradient_next_iterate_too_close()
    assert np.array_equal(b.approx_inv_hessian(), h)
    b.close()


# ---- iterate-sequence parity ----
@pytest.mark.parametrize("memoize", [0, 1])
@pytest.mark.parametrize("name", list(BC.WINDOWS))
def test_window_parity(qn, qo, name, memoize):
    w = BC.WINDOWS[name]
    pr = BC.problem(w, qo)
    ref, o, _ = BC.run_ref(pr, w["ls"], w["K"])
    orc = _Oracle(qn, w, pr)
    try:
        s, status = _run(qn, w, pr, orc.oracle, w["K"], memoize)
        tr, xs = s.trace()
        st = s.stats()
        tol = BC.tolerance(w)
        print(f"{name} memoize={memoize}: k={s.k()} calls={st['oracle_calls']}/{o.calls} evals={st['oracle_evals']}/{o.evals} path={st['path']}")
        assert status == "max_iter" and s.k() == w["K"] == len(tr)
        ok = _close("x-trace", xs, np.array(ref.trace_x), tol)
        ok &= _close("f", [r["f"] for r in tr], [r["f"] for r in ref.trace], tol)
        ok &= _close("s_norm", [r["s_norm"] for r in tr], [r["s_norm"] for r in ref.trace], tol)
        ok &= _close("y_norm", [r["y_norm"] for r in tr], [r["y_norm"] for r in ref.trace], tol)
        ok &= _close("H", s.approx_inv_hessian(), ref.h, tol)
        assert ok
        assert [r["updated"] for r in tr] == [r["updated"] for r in ref.trace]
        assert [r["n_evals"] for r in tr] == [r["n_evals"] for r in ref.trace]
        assert st["oracle_calls"] == o.calls
        assert st["oracle_evals"] == (o.evals if memoize else o.calls)
        if orc.chain and not memoize:
            assert orc.chain.calls() == o.calls
        if pr["lb"] is not None:  # inside the box exactly
            assert np.all(xs >= pr["lb"]) and np.all(xs <= pr["ub"])
        n_pad = (w["n"] + 15) // 16 * 16
        if w["n"] > 5:
            assert st["path"] & qn._abi.PATH_RANK1
            assert not st["path"] & (qn._abi.PATH_FUSED | qn._abi.PATH_SYM | qn._abi.PATH_SYM_GENERIC | qn._abi.PATH_SYM2 | qn._abi.PATH_PIPELINED)
            K = w["K"]
            # memoize = 1: one direction pass for the very first iteration, then ONE pass per iteration; memoize = 0: two per iteration
            assert st["h_passes"] == (K + 1 if memoize else 2 * K)
            rw = K - 1  # passes that found an update pending and wrote H back
            assert st["h_bytes"] == (st["h_passes"] + rw) * n_pad * n_pad * 8
            # padding stays exactly zero, the logical part is what the getter returned: nothing else to check from outside
        else:
            assert not st["path"] & qn._abi.PATH_RANK1
        s.close()
    finally:
        orc.close()


@pytest.mark.parametrize("name,ls,bounded", BC.REFERENCE_TESTS)
def test_reference_tests_on_the_gpu(qn, name, ls, bounded):
    pr = dict(fn=BC.two_var(1.0), x0=BC.X0_2D.copy(), lb=-BC.INF2 if bounded else None, ub=BC.INF2 if bounded else None)
    ref, o, _ = BC.run_ref(pr, ls, 1000, max_ls=100000)
    s = _solver(qn, pr)
    s.minimize(_line_search(qn, ls, pr["lb"], pr["ub"], 2), pr["fn"], 1000, 100000)
    f, g = pr["fn"](s.x())
    assert abs(f - 0.0) < 1e-6 and s.has_converged((f, g))
    assert s.k() == ref.k and s.stats()["oracle_calls"] == o.calls
    assert np.array_equal(s.x(), ref.x)  # n <= 5: the reference's operation order
    s.close()


def test_skip_rule_and_convergence(qn, qo):
    w = BC.SKIP_CASE
    pr = BC.problem(w, qo)
    ref, o, _ = BC.run_ref(pr, w["ls"], w["K"])
    s, status = _run(qn, w, pr, pr["fn"], w["K"], 0)
    tr, _ = s.trace()
    assert status == "ok" and s.k() == ref.k
    assert [r["updated"] for r in tr] == [r["updated"] for r in ref.trace] and tr[-1]["updated"] == 0
    assert s.next_iterate_too_close() and s.s_norm() < BC.TOL
    assert BC.rel_diff(s.approx_inv_hessian(), ref.h) <= BC.tolerance(w)
    s.close()


def test_determinism(qn, qo):
    w = BC.WINDOWS["q384_bt"]
    pr = BC.problem(w, qo)
    obj = qn.Quadratic(*pr["data"])
    runs = []
    for _ in range(2):
        s, _ = _run(qn, w, pr, obj, w["K"], 1)
        runs.append((s.x().tobytes(), s.approx_inv_hessian().tobytes()))
        s.close()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("name", ["q130_mt", "two_var_mt"])
def test_warm_restart_and_reset(qn, qo, name):
    w = BC.WINDOWS[name]
    pr = BC.problem(w, qo)
    orc = _Oracle(qn, w, pr)
    K = w["K"]
    # (memoize = 0: a new call evaluates at x and forms d = -H g by a pass over H, as every iteration of such a run does; with memoize = 1 the
    # iterations inside one call form their directions lazily from the update pass's sums -- the same numbers to rounding, not to the bit)
    one, _ = _run(qn, w, pr, orc.oracle, K, 0)
    two = _solver(qn, pr)
    for _ in range(2):
        two, status = _run(qn, w, pr, orc.oracle, K // 2, 0, s=two)
        assert status == "max_iter" and two.k() == K // 2
    assert one.x().tobytes() == two.x().tobytes()
    assert one.approx_inv_hessian().tobytes() == two.approx_inv_hessian().tobytes()
    assert one.s_norm() == two.s_norm() and one.y_norm() == two.y_norm()
    two.reset(pr["x0"])
    assert np.array_equal(two.approx_inv_hessian(), np.eye(w["n"])) and two.k() == 0
    assert two.s_norm() is None and two.y_norm() is None
    one.close()
    two.close()
    orc.close()


def test_rejections(qn):
    s = qn.Broyden(1e-8, np.ones(7))
    with pytest.raises(qn.ErrorInputParams):
        s.minimize(qn.GLLQuadratic(1e-4, 10), lambda x: (0.5 * float(x @ x), x), 5, 5)
    s.close()


def test_world_above_one_is_rejected(qn):
    """ranks as threads, as tests/test_gpu_partitions.py"""
    from thread_ranks import run_ranks

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        with pytest.raises(qn.ErrorInputParams, match="world > 1"):
            qn.Broyden(1e-6, np.zeros(32), ctx=ctx)
        qn.GradientDescent(1e-6, np.zeros(32), ctx=ctx).close()  # (the context itself is fine)
        ctx.close()
        return True
    assert run_ranks(2, body, timeout=60.0) == [True, True]


def test_callback_sees_every_iteration(qn, qo):
    w = BC.WINDOWS["q130_mt"]
    pr = BC.problem(w, qo)
    ref, _, _ = BC.run_ref(pr, w["ls"], w["K"])
    seen = []
    s = _solver(qn, pr)
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.MoreThuente(), qn.Quadratic(*pr["data"]), w["K"], BC.MAX_LS, callback=lambda me: seen.append((me.k(), me.s_norm())))
    assert [k for k, _ in seen] == list(range(1, w["K"] + 1))
    assert BC.rel_diff([v for _, v in seen], [r["s_norm"] for r in ref.trace]) <= BC.tolerance(w)
    s.close()


# ---- mirrors ----
def test_broyden_example_cpp():
    exe = os.path.join(ROOT, "examples", "broyden_example.bin")
    assert os.path.exists(exe), "examples/broyden_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Convergence: true" in p.stdout and p.stdout.strip().endswith("broyden example ok")


def test_python_getters_round_trip(qn):
    x0 = np.array([3.0, -0.25, 0.5, 9.0, -4.0, 0.0, 1.0])
    s = qn.Broyden.new(1e-9, x0)
    assert np.array_equal(s.x(), x0) and np.array_equal(s.xk(), x0) and s.k() == 0 and s.tol() == 1e-9
    assert s.s_norm() is None and s.y_norm() is None and not s.next_iterate_too_close() and not s.gradient_next_iterate_too_close()
    assert np.array_equal(s.identity(), np.eye(7)) and np.array_equal(s.approx_inv_hessian(), np.eye(7))
    lb, ub = np.full(7, -1.0), np.full(7, 1.0)
    b = qn.BroydenB.new(1e-9, x0, lb, ub)
    assert np.array_equal(b.x(), np.clip(x0, -1.0, 1.0))  # x0.box_projection, broyden_b.rs:51
    assert np.array_equal(b.lower_bound(), lb) and np.array_equal(b.upper_bound(), ub)
    g = np.linspace(-2.0, 2.0, 7)
    assert np.array_equal(b.compute_direction((0.0, g)), np.clip(b.x() - g, lb, ub) - b.x())  # H = I: P(x - g) - x
    s.close()
    b.close()
