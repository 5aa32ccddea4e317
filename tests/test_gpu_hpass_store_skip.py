"""GPU tests of the update pass that stores every second time (csrc/qn_sym2.hip.h s2_hpass_kernel, set_option("hpass_store_skip", v)).

With the option on (the default) an update pass that finds ONE update pending applies it in registers, forms its sums on the result and does not store H
(the read pass); the next pass applies that update and then the newer one to the same stored H and stores (the write pass).  Per element these are the
operations of two storing passes in the same order, so nothing may differ from option 0 (every pass stores): the iterates, the trace, the counters and
the whole inverse Hessian are compared bit for bit -- inside a call, across calls that end after either kind of pass, and through everything that
reads H or the pending vectors outside a call.  qn_stats.n_hpass_nostore counts the read passes, h_bytes_moved what the passes really moved.

Shapes: n = 1024 (the smallest on the second-generation path: 8 block-rows, lists longer than two items, no slivers) and n = 4096 (the smallest with
row slivers, the pair lists and the touch workgroups).  The objective is the seeded quadratic of tests/problems.py.

Which passes do not store, from the rules: a cold call runs one direction pass (nothing pending: it stores) and then one update pass per iteration;
update pass j = 1, 2, 3, ... of a run finds 0, 1, 2, 1, 2, ... updates pending, so the even ones are read passes.  A run of K iterations from a cold
start has K // 2 of them and ends with two updates pending exactly when K is even (K >= 2); a warm call goes on where the count stood."""
import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

NEW_COUNTERS = ("n_hpass_nostore", "h_bytes_moved")
_objs = {}


def _problem(qn, n, kappa=1e3):
    if (n, kappa) not in _objs:
        diag = P.synth_diag(n, kappa)
        b, x0 = P.synth_vectors(n)
        _objs[(n, kappa)] = (qn.Quadratic.synthetic(n, P.SEED, diag, b), x0)
    return _objs[(n, kappa)]


def _ls(qn, lsname):
    return qn.MoreThuente() if lsname == "mt" else qn.BackTracking(1e-4, 0.5)


def _solver(qn, method, x0, skip, sync=0, tol=1e-10, trace=20, opts=()):
    s = (qn.BFGS if method == "bfgs" else qn.DFP)(tol, x0)
    s.set_trace(trace, with_x=True)
    s.configure("hpass_store_skip", skip)
    for name, v in opts:
        s.configure(name, v)
    s.set_sync_mode(sync)
    return s


def _minimize(qn, s, ls, obj, iters, ls_iters=20):
    try:
        s.minimize(ls, obj, iters, ls_iters)
    except qn.MaxIterReached:
        return 1
    except qn.SolverError as e:  # (any other status: compared by its type)
        return type(e).__name__
    return 0


def _same_stats(a, b):
    for k in a:
        if k not in NEW_COUNTERS and not k.startswith("t_") and not k.endswith("_timed"):
            assert a[k] == b[k], (k, a[k], b[k])


def _same_state(a, b, with_h=True):
    (tr_a, xs_a), (tr_b, xs_b) = a.trace(), b.trace()
    assert tr_a == tr_b and np.array_equal(xs_a, xs_b)
    assert a.k() == b.k() and np.array_equal(a.x(), b.x())
    _same_stats(a.stats(), b.stats())
    if with_h:
        assert np.array_equal(a.approx_inv_hessian(), b.approx_inv_hessian())


def _expected_nostore(passes_with_pending):
    """read passes among update passes that find `passes_with_pending` = [0, 1, 2, 1, ...] updates pending"""
    return sum(1 for c in passes_with_pending if c == 1)


def _pending_sequence(count, n_update_passes):
    """the counts the next update passes find, starting from `count`; returns (list, count afterwards)"""
    seq = []
    for _ in range(n_update_passes):
        seq.append(count)
        count = {0: 1, 1: 2, 2: 1}[count]
    return seq, count


# 1 ---- the same bits as storing every pass
@pytest.mark.parametrize("iters", [1, 2, 3, 4, 5, 20])
@pytest.mark.parametrize("sync", [0, 1], ids=["pipelined", "sync"])
@pytest.mark.parametrize("lsname", ["mt", "bt"])
@pytest.mark.parametrize("method", ["bfgs", "dfp"])
@pytest.mark.parametrize("n", [1024, 4096])
def test_same_bits_as_storing_every_pass(qn, n, method, lsname, sync, iters):
    obj, x0 = _problem(qn, n)
    runs = []
    for skip in (0, 1):
        s = _solver(qn, method, x0, skip, sync)
        st = _minimize(qn, s, _ls(qn, lsname), obj, iters)
        runs.append((s, st, s.stats()))
    (off, st0, stats0), (on, st1, stats1) = runs
    assert stats0["path"] & 16 and stats1["path"] & 16  # QN_PATH_SYM2
    assert st0 == st1
    seq, _ = _pending_sequence(0, stats0["h_passes"] - 1)  # (the direction pass of the cold start aside)
    print("n_hpass_nostore off / on:", stats0["n_hpass_nostore"], stats1["n_hpass_nostore"], "h_passes:", stats0["h_passes"])
    assert stats0["n_hpass_nostore"] == 0
    assert stats1["n_hpass_nostore"] == _expected_nostore(seq)
    _same_state(on, off)


# 2 ---- continuation: the count is carried from call to call
@pytest.mark.parametrize("split", [(3, 4), (5, 5), (2, 1, 2)], ids=["3+4", "5+5", "2+1+2"])
@pytest.mark.parametrize("n,read_h", [(1024, False), (4096, False), (1024, True)], ids=["1024-x-per-call", "4096-x-per-call", "1024-x-and-H-per-call"])
def test_continuation_across_calls(qn, n, split, read_h):
    """read_h False: only x is read between the calls, so a call may start with one or two updates pending (the last call's H is compared);
    True: H is read after every call too (the getter applies what is pending: every call then starts from a current H).  (The getter's passes are the
    generic kernel at either size and it moves 134 MB to the host at n = 4096: after every call at n = 1024 only; test_getter_after_two_pending has 4096.)"""
    obj, x0 = _problem(qn, n)
    total = sum(split)
    one = _solver(qn, "bfgs", x0, 1, trace=total)
    _minimize(qn, one, qn.MoreThuente(), obj, total)
    legs = {}
    for skip in (0, 1):
        s = _solver(qn, "bfgs", x0, skip, trace=total)
        ls = qn.MoreThuente()
        out, count = [], 0
        for leg, iters in enumerate(split):
            st = _minimize(qn, s, ls, obj, iters)
            stats = s.stats()
            h = s.approx_inv_hessian() if read_h else None
            if skip:
                cold = leg == 0 or read_h
                seq, count = _pending_sequence(0 if cold else count, stats["h_passes"] - (1 if cold else 0))
                assert stats["n_hpass_nostore"] == _expected_nostore(seq), (leg, seq, stats["n_hpass_nostore"])
            out.append((st, s.x(), stats, h))
        legs[skip] = (out, s.approx_inv_hessian(), s)
    for (st0, x_0, stats0, h0), (st1, x_1, stats1, h1) in zip(legs[0][0], legs[1][0]):
        assert st0 == st1 and np.array_equal(x_0, x_1)
        if not read_h:
            assert stats0["launches"] == stats1["launches"]  # (no launch added to carry the count)
        # (read_h: qn_stats.launches also counts the getter's passes between the calls -- one per pending update, so one more where a call ended with two)
        _same_stats({k: v for k, v in stats0.items() if k != "launches"}, {k: v for k, v in stats1.items() if k != "launches"})
        if read_h:
            assert np.array_equal(h0, h1)
    assert np.array_equal(legs[0][1], legs[1][1])
    if not read_h:  # the calls together are the one call of the sum (warm continuation: nothing is evaluated or multiplied twice)
        assert np.array_equal(legs[1][2].x(), one.x())
        assert np.array_equal(legs[1][1], one.approx_inv_hessian())


# 3 ---- everything that reads H or the pending vectors outside a call
def _two_pending_run(qn, n, skip, method="bfgs"):
    obj, x0 = _problem(qn, n)
    iters = 4  # (even: update passes find 0, 1, 2, 1 pending -- the last one does not store, the call ends with two)
    s = _solver(qn, method, x0, skip)
    ls = qn.MoreThuente()
    _minimize(qn, s, ls, obj, iters)
    seq, count = _pending_sequence(0, s.stats()["h_passes"] - 1)
    assert count == 2 and seq[-1] == 1
    assert s.stats()["n_hpass_nostore"] == (_expected_nostore(seq) if skip else 0)
    return s, ls, obj, x0


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("method", ["bfgs", "dfp"])
def test_getter_after_two_pending(qn, n, method):
    a, *_ = _two_pending_run(qn, n, 0, method)
    b, *_ = _two_pending_run(qn, n, 1, method)
    ha = a.approx_inv_hessian()
    hb = b.approx_inv_hessian()
    assert np.array_equal(ha, hb)
    if n == 1024:
        assert np.array_equal(hb, b.approx_inv_hessian())  # (and nothing is applied twice)


@pytest.mark.parametrize("n", [1024, 4096])
def test_reset_after_two_pending(qn, n):
    outs = []
    for skip in (0, 1):
        s, ls, obj, x0 = _two_pending_run(qn, n, skip)
        s.reset(x0)
        s.set_trace(20, with_x=True)
        _minimize(qn, s, ls, obj, 5)
        outs.append(s)
    _same_state(outs[1], outs[0])
    fresh = _solver(qn, "bfgs", _problem(qn, n)[1], 1)
    _minimize(qn, fresh, qn.MoreThuente(), _problem(qn, n)[0], 5)
    assert np.array_equal(fresh.x(), outs[1].x())
    if n == 1024:
        assert np.array_equal(fresh.approx_inv_hessian(), outs[1].approx_inv_hessian())


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("option", ["second_generation", "hpass_store_skip"])
def test_path_or_option_change_after_two_pending(qn, n, option):
    """five more iterations on the first-generation kernels (or with every pass storing) from where the call left off"""
    outs = []
    for skip in (0, 1):
        s, ls, obj, _ = _two_pending_run(qn, n, skip)
        s.set_option(option, 0)
        st = _minimize(qn, s, ls, obj, 5)
        outs.append((st, s.x(), s.k(), s.trace(), s.approx_inv_hessian(), s.stats()))
    a, b = outs
    assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])
    assert a[3][0] == b[3][0] and np.array_equal(a[3][1], b[3][1])
    assert np.array_equal(a[4], b[4])
    assert b[5]["n_hpass_nostore"] == 0
    for k in ("oracle_evals", "h_passes", "iterations", "h_bytes"):
        assert a[5][k] == b[5][k], k


@pytest.mark.parametrize("n", [1024, 4096])
def test_trait_hooks_after_two_pending(qn, n):
    """compute_direction, set_x and secant_update (the sequence of tests/test_gpu_trait_hooks.py's template) on the state the call left"""
    rng = np.random.Generator(np.random.Philox(key=7))
    g, y = rng.standard_normal(n), rng.standard_normal(n)
    outs = []
    for skip in (0, 1):
        s, *_ = _two_pending_run(qn, n, skip)
        d = s.compute_direction((0.0, g))
        x = s.x()
        step = 0.5 * d
        s.set_x(x + step)
        s.secant_update(step, y + 2.0 * step)  # (s'y > 0 by construction is not needed: the same arithmetic on both sides)
        d2 = s.compute_direction((0.0, g))
        outs.append((d, d2, s.x(), s.approx_inv_hessian()))
    for u, v in zip(*outs):
        assert np.array_equal(u, v)


# 4 ---- ends that are not the cap
def test_converged_run(qn):
    n = 1024
    obj, x0 = _problem(qn, n, kappa=10.0)
    outs = []
    for skip in (0, 1):
        s = _solver(qn, "bfgs", x0, skip, tol=1e-6, trace=200)
        st = _minimize(qn, s, qn.MoreThuente(), obj, 200)
        outs.append((s, st))
    (a, st0), (b, st1) = outs
    assert st0 == st1 == 0
    print("converged after", b.k(), "iterations; read passes:", b.stats()["n_hpass_nostore"])
    assert b.stats()["n_hpass_nostore"] > 0
    _same_state(b, a)


@pytest.mark.parametrize("n", [1024, 4096])
def test_run_ended_by_the_line_search(qn, n):
    obj, x0 = _problem(qn, n)
    outs = []
    for skip in (0, 1):
        s = _solver(qn, "bfgs", x0, skip)
        st = _minimize(qn, s, qn.MoreThuente(), obj, 20, ls_iters=1)
        outs.append((s, st))
    (a, st0), (b, st1) = outs
    assert st0 == st1
    _same_state(b, a)


# 5 ---- counting
@pytest.mark.parametrize("n", [1024, 4096])
def test_counters(qn, n):
    obj, x0 = _problem(qn, n)
    stats = []
    for skip in (0, 1):
        s = _solver(qn, "bfgs", x0, skip)
        _minimize(qn, s, qn.MoreThuente(), obj, 20)
        stats.append(s.stats())
    off, on = stats
    seq, _ = _pending_sequence(0, off["h_passes"] - 1)
    assert on["h_passes"] == off["h_passes"]
    assert on["n_hpass_nostore"] == _expected_nostore(seq) == (off["h_passes"] - 1) // 2
    assert on["h_bytes"] == off["h_bytes"] == 2 * off["h_passes"] * off["matrix_bytes_per_pass"]
    assert off["h_bytes_moved"] == off["h_bytes"]
    assert on["h_bytes_moved"] == on["h_bytes"] - on["n_hpass_nostore"] * on["matrix_bytes_per_pass"]


# 6 ---- the variants that keep at most one update pending
@pytest.mark.parametrize("option", ["tail_reduce", "folded_accept_reduce"])
def test_excluded_single_rank_variants(qn, option):
    n = 1024
    obj, x0 = _problem(qn, n)
    outs = []
    for skip in (0, 1):
        s = _solver(qn, "bfgs", x0, skip, opts=((option, 1),))
        _minimize(qn, s, qn.MoreThuente(), obj, 12)
        outs.append(s)
    assert outs[0].stats()["n_hpass_nostore"] == 0 and outs[1].stats()["n_hpass_nostore"] == 0
    assert outs[1].stats()["h_bytes_moved"] == outs[1].stats()["h_bytes"]
    _same_state(outs[1], outs[0])


def test_excluded_bounded_run(qn):
    n = 1024
    obj, x0 = _problem(qn, n)
    lb, ub = x0 - 0.3, x0 + 0.3
    outs = []
    for skip in (0, 1):
        s = qn.BFGSB.new(1e-9, x0, lb, ub)
        s.set_trace(12, with_x=True)
        s.configure("hpass_store_skip", skip)
        ls = qn.MoreThuenteB.new(n).with_lower_bound(lb).with_upper_bound(ub)
        _minimize(qn, s, ls, obj, 12, ls_iters=30)
        outs.append(s)
    assert outs[0].stats()["path"] & 16
    assert outs[0].stats()["n_hpass_nostore"] == 0 and outs[1].stats()["n_hpass_nostore"] == 0
    _same_state(outs[1], outs[0])


def test_excluded_two_rank_partition(qn):
    from thread_ranks import run_ranks
    n, world, iters = 1024, 2, 6
    diag = P.synth_diag(n)
    b, x0 = P.synth_vectors(n)

    def run(skip):
        def body(rank, world_, group):
            ctx = qn.Context(0, rank=rank, world=world_, host_allgather=group.allgather_fn(rank))
            ctx.comm_check()
            obj = qn.Quadratic.synthetic(n, P.SEED, diag, b, ctx=ctx)
            s = qn.BFGS(1e-10, x0, ctx=ctx)
            s.set_trace(iters, with_x=True)
            s.configure("hpass_store_skip", skip)
            _minimize(qn, s, qn.MoreThuente(), obj, iters)
            st = s.stats()
            out = {"x": s.x(), "tr": s.trace()[0], "nostore": st["n_hpass_nostore"], "launches": st["launches"], "h_bytes": st["h_bytes"],
                   "h": s.approx_inv_hessian(all_ranks=True)}
            group.sync()
            s.close(); obj.close(); ctx.close()
            return out
        return run_ranks(world, body)

    off, on = run(0), run(1)
    for a, c in zip(off, on):
        assert a["nostore"] == 0 and c["nostore"] == 0
        assert a["tr"] == c["tr"] and np.array_equal(a["x"], c["x"]) and np.array_equal(a["h"], c["h"])
        assert a["launches"] == c["launches"] and a["h_bytes"] == c["h_bytes"]
