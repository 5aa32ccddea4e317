"""GPU tests of buffer ownership: every device and pinned buffer of the host layer belongs to one DevBuf / PinnedBuf owner, and the owners
count what they hold (qn_debug_live_allocations: live allocations and live bytes, process-wide).  Each case reads the counter, builds its
objects, runs far enough to reach the lazy allocations it names, closes everything and wants the counter back where it was -- "destroy
released what the run allocated".  The shapes are the smallest that reach each allocation."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu
PATH_FUSED, PATH_SYM, PATH_SYM2 = 1, 2, 16


def _live(qn):
    fn = qn._abi.lib().qn_debug_live_allocations  # diagnostics: exported, not declared in include/qn_hip.h
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    count, nbytes = C.c_size_t(), C.c_size_t()
    assert fn(C.byref(count), C.byref(nbytes)) == 0
    return count.value, nbytes.value


@contextlib.contextmanager
def _nothing_left(qn):
    """yields a fresh context and a list; the body appends what it builds; all of it is closed, then the counter is back"""
    gc.collect()
    before = _live(qn)
    ctx, made = qn.Context(0), []
    try:
        yield ctx, made
        held = _live(qn)
        print(f"    held at the end of the body: {held[0] - before[0]} allocations, {held[1] - before[1]} bytes")
        assert held[0] > before[0] and held[1] > before[1]  # (the counter sees the library's buffers at all)
    finally:
        for obj in reversed(made):
            obj.close()
        ctx.close()
    gc.collect()
    assert _live(qn) == before


def _run(qn, s, ls, oracle, iters, max_ls=20):
    try:
        s.minimize(ls, oracle, iters, max_ls)
    except qn.MaxIterReached:
        pass
    return s.stats()["path"]


def _spd(n, seed=7):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n)) / n
    q = 0.5 * (m + m.T) + np.diag(P.synth_diag(n, 1e2))
    b, x0 = P.synth_vectors(n)
    return q, b, x0


def _closure(qn, q, b, hessian=False):
    def fn(x):
        qx = q @ x
        fe = qn.FuncEvalMultivariate(0.5 * float(x @ qx) - float(b @ x), qx - b)
        return fe.with_hessian(q) if hessian else fe
    return fn


def test_second_generation_symmetric_path(qn):
    n, iters = 1024, 6
    diag = P.synth_diag(n)
    b, x0 = P.synth_vectors(n)
    with _nothing_left(qn) as (ctx, made):
        obj = qn.Quadratic.synthetic(n, P.SEED, diag, b, ctx=ctx)
        s = qn.BFGS(1e-10, x0, ctx=ctx)
        made += [obj, s]
        s.set_trace(iters, with_x=True)
        path = _run(qn, s, qn.MoreThuente(), obj, iters)  # (its first run also measures H's placement: place_h's candidates)
        assert path & PATH_SYM2 and path & PATH_SYM, path
        after_first = _live(qn)
        # reset and run again: reallocation replaces a buffer, it does not add one
        s.reset(x0)
        assert _run(qn, s, qn.MoreThuente(), obj, iters) & PATH_SYM2
        assert _live(qn) == after_first
        s.set_option("tail_reduce", 1)  # the block-rows' arrival counters
        assert _run(qn, s, qn.MoreThuente(), obj, iters) & PATH_SYM2
        assert _live(qn)[0] == after_first[0] + 1
        s.set_option("second_generation", 0)  # the first-generation tile kernels: their slot buffer exists since the first symmetric run
        path = _run(qn, s, qn.MoreThuente(), obj, iters)
        assert path & PATH_SYM and not path & PATH_SYM2, path
        assert _live(qn)[0] == after_first[0] + 1


def test_second_generation_path_on_logsumexp(qn):
    m, n = 256, 1024
    rng = np.random.default_rng(11)
    a = rng.standard_normal((m, n)) * (2.0 / np.sqrt(n))
    c, x0 = rng.standard_normal(m), rng.standard_normal(n)
    with _nothing_left(qn) as (ctx, made):
        obj = qn.LogSumExp(a, c, 0.1, ctx=ctx)  # (the one-pass evaluation's buffers)
        s = qn.BFGS(1e-10, x0, ctx=ctx)
        made += [obj, s]
        s.set_trace(6, with_x=True)
        assert _run(qn, s, qn.MoreThuente(), obj, 6) & PATH_SYM2  # (the generic objectives' second table of per-workgroup sums)
        obj(x0)  # ... and the evaluation scratch of the objective called on its own


def test_fused_row_kernels_and_retiling(qn):
    n = 256
    diag = P.synth_diag(n)
    b, x0 = P.synth_vectors(n)
    with _nothing_left(qn) as (ctx, made):
        obj = qn.Quadratic.synthetic(n, P.SEED, diag, b, ctx=ctx)
        s = qn.BFGS(1e-10, x0, ctx=ctx)
        made += [obj, s]
        s.set_option("symmetric_storage", 0)
        path = _run(qn, s, qn.MoreThuente(), obj, 6)
        assert path & PATH_FUSED and not path & PATH_SYM, path
        count = _live(qn)[0]
        s.set_tiling(8, 2)  # hp / q for two column splits (which the generic kernels serve): replaced, not added
        assert not _run(qn, s, qn.MoreThuente(), obj, 6) & PATH_FUSED
        assert _live(qn)[0] == count
        s.set_tiling(8, 1)  # ... and back on the row kernels with 8-row tiles: hp / q now, evp / hpp at the run
        assert _run(qn, s, qn.MoreThuente(), obj, 6) & PATH_FUSED
        assert _live(qn)[0] == count


@pytest.mark.parametrize("n", [64, 3])
def test_generic_path_host_closure(qn, n):
    q, b, x0 = _spd(n)
    with _nothing_left(qn) as (ctx, made):
        s = qn.BFGS(1e-10, x0, ctx=ctx)
        made.append(s)
        s.set_trace(6, with_x=True)
        assert not _run(qn, s, qn.MoreThuente(), _closure(qn, q, b), 6) & PATH_FUSED


def test_generic_path_bounded(qn):
    n = 64
    q, b, x0 = _spd(n)
    lb, ub = np.full(n, -0.5), np.full(n, 0.5)
    with _nothing_left(qn) as (ctx, made):
        s = qn.BFGSB(1e-10, x0, lb, ub, ctx=ctx)
        made.append(s)
        _run(qn, s, qn.MoreThuenteB(n).with_lower_bound(lb).with_upper_bound(ub), _closure(qn, q, b), 6)


@pytest.mark.parametrize("n,lu", [(100, False), (100, True), (600, False)])
def test_newton_with_host_hessian(qn, n, lu):
    """n = 100: Cholesky, and the pivoted LU with its panel, counter and record buffers; n = 600: the 512-wide blocks' inverses"""
    q, b, x0 = _spd(n)
    with _nothing_left(qn) as (ctx, made):
        s = qn.Newton(1e-8, x0, ctx=ctx)
        made.append(s)
        if lu:
            s.set_option("newton_pivoted_lu", 1)
            s.set_option("lu_split_min_rows", 0)
        _run(qn, s, qn.MoreThuente(), _closure(qn, q, b, hessian=True), 2)
        assert np.linalg.norm(q @ s.x() - b) <= 1e-6 * np.linalg.norm(b)  # (the direction really was Newton's: a quadratic, solved in one step)


@pytest.mark.parametrize("family", ["spg", "pgd", "pnewton"])
def test_first_order_family(qn, family):
    n = 64
    q, b, x0 = _spd(n)
    lb, ub = np.full(n, -0.5), np.full(n, 0.5)
    with _nothing_left(qn) as (ctx, made):
        fn = _closure(qn, q, b, hessian=family == "pnewton")
        if family == "spg":
            s, ls = qn.SpectralProjectedGradient(1e-10, x0, fn, lb, ub, ctx=ctx), qn.GLLQuadratic(1e-4, 10)
        elif family == "pgd":
            s, ls = qn.ProjectedGradientDescent(1e-10, x0, lb, ub, ctx=ctx), qn.BackTrackingB(1e-4, 0.5, lb, ub)
        else:
            s, ls = qn.ProjectedNewton(1e-10, x0, lb, ub, ctx=ctx), qn.GLLQuadratic(1e-4, 10)
        made.append(s)
        _run(qn, s, ls, fn, 5, 50)


def test_broyden(qn):
    n = 200
    q, b, x0 = _spd(n)
    with _nothing_left(qn) as (ctx, made):
        s = qn.Broyden(1e-10, x0, ctx=ctx)
        made.append(s)
        _run(qn, s, qn.MoreThuente(), _closure(qn, q, b), 5)


def test_trait_hook_temporaries(qn):
    n = 64
    q, b, x0 = _spd(n)
    with _nothing_left(qn) as (ctx, made):
        s = qn.BFGS(1e-10, x0, ctx=ctx)
        made.append(s)
        count = _live(qn)[0]
        g = q @ x0 - b
        d = s.compute_direction((0.0, g))
        assert np.array_equal(d, -g)  # H = I
        sk = 1e-2 * d
        s.secant_update(sk, q @ sk)
        h = s.approx_inv_hessian()
        s.set_approx_inv_hessian(h)
        assert _live(qn)[0] == count  # the calls' temporaries went with the calls


def test_partial_construction_is_released(qn):
    """n = 2^20: the 8 TiB inverse Hessian is refused at once (an allocation error code, no fault); the handle is already stored in *out, as the
    callers rely on, and destroying it releases what was constructed before the failure."""
    A = qn._abi
    n = 1 << 20
    x0 = np.zeros(n)
    gc.collect()
    before = _live(qn)
    ctx = qn.Context(0)
    h = C.c_void_p()
    status = A.lib().qn_solver_create(ctx.h, A.BFGS, 1e-8, x0.ctypes.data_as(A.dp), n, C.byref(h))
    assert status == A.ABNORMAL_TERMINATION, (status, A.lib().qn_last_error_message())
    assert b"hipMalloc" in A.lib().qn_last_error_message()
    assert h.value
    A.lib().qn_solver_destroy(h)
    ctx.close()
    assert _live(qn) == before
