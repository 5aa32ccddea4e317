"""GPU: the log-sum-exp evaluation inside DFP / BFGS runs, held to the extended-precision truth and bounds of tests/lse_eval_cases.py (licensed on the
CPU by tests/test_ref_lse_eval.py) -- on the second-generation structure (s2g_onepass / s2g_combine / s2g_vec, pipelined and synchronous, bit-equal),
on the generic path (lse_onepass / lse_combine / lse_finish1), row-sharded on 2, 3 and 4 ranks (ranks as threads, every rank the same bits), and
stand-alone obj(x) in the one-pass and the two-pass form.  The cases reach what the parity tests' benign data does not: rescale factors that underflow
to 0 or nearly, a maximum that rises or falls at every row, ranks and workgroups without rows, m = 1 and m = 5, every KCH instance of the pass, and
masked rows (c_k = -inf), which contribute nothing wherever they fall in the grid.  Every run is replayed iteration by iteration from its own recorded
iterates: f, gnorm, s_norm, y_norm and, entry by entry, the step against -t H_k g_k.

With the select of the two row loops taken out again (exp(m_run - m_new) with both -inf) the masked cases fail: f of iteration 0 is NaN."""
import numpy as np
import pytest

import lse_eval_cases as E
from thread_ranks import run_ranks

pytestmark = pytest.mark.gpu

TALLY = E.Tally()
WORST = {}       # family -> worst asserted ratio of the runs' replays
WORST_OBJ = {}   # family -> worst ratio of the stand-alone evaluations
_truths = {}     # case -> {bytes of x: Truth}

SINGLE = [c for c in E.CASES if 1 in c.worlds]
METHODS = [("dfp", "mt"), ("dfp", "bt"), ("bfgs", "mt"), ("bfgs", "bt")]


def _ls(qn, lsname):
    return qn.MoreThuente() if lsname == "mt" else qn.BackTracking(1e-4, 0.5)


def _solve(qn, cs, method, lsname, obj, ctx=None, option=None, sync=None):
    """one run of the case: (trace records, recorded iterates, path); OK and MaxIterReached are the valid endings"""
    x0 = E.problem(cs.name)[2]
    s = (qn.DFP if method == "dfp" else qn.BFGS)(1e-10, x0, **({"ctx": ctx} if ctx is not None else {}))
    try:
        s.set_trace(cs.iters, with_x=True)
        if option:
            s.configure(*option)
        if sync is not None:
            s.set_sync_mode(sync)
        try:
            s.minimize(_ls(qn, lsname), obj, cs.iters, 20)
        except qn.MaxIterReached:
            pass
        tr, xs = s.trace()
        return tr, np.array(xs), s.stats()["path"]
    finally:
        s.close()  # (also when the run fails: a solver must not outlive its context, and a failed rank's frames are collected in no particular order)


def _same_bits(run_a, run_b):
    (tr_a, xs_a, _), (tr_b, xs_b, _) = run_a, run_b
    if len(tr_a) != len(tr_b) or xs_a.shape != xs_b.shape or not np.array_equal(xs_a, xs_b, equal_nan=True):
        return False
    for ra, rb in zip(tr_a, tr_b):
        if ra.keys() != rb.keys() or not all(np.array_equal(ra[k], rb[k], equal_nan=True) for k in ra):
            return False
    return True


def _replay(cs, method, tag, run):
    a, c, x0 = E.problem(cs.name)
    tr, xs, _ = run
    assert len(tr) >= 1, (cs.name, tag, "the run left no trace record")
    rep = E.replay(f"{cs.name}/{method}/{tag}", a, c, x0, method, tr, xs, truth_cache=_truths.setdefault(cs.name, {}))
    E.check(rep)
    TALLY.add(rep)
    WORST[cs.label] = max(WORST.get(cs.label, 0.0), rep.worst)


@pytest.mark.parametrize("method,lsname", METHODS)
@pytest.mark.parametrize("cs", SINGLE, ids=repr)
def test_runs_replay_on_the_second_generation_structure_and_on_the_generic_path(qn, cs, method, lsname):
    a, c, _ = E.problem(cs.name)
    obj = qn.LogSumExp(a, c, E.MU)
    try:
        pipelined = _solve(qn, cs, method, lsname, obj, sync=0)
        synchronous = _solve(qn, cs, method, lsname, obj, sync=1)
        generic = _solve(qn, cs, method, lsname, obj, option=("second_generation", 0))
    finally:
        obj.close()
    assert pipelined[2] & 16 and synchronous[2] & 16 and not generic[2] & 16, (pipelined[2], synchronous[2], generic[2])
    assert _same_bits(pipelined, synchronous)  # pipelined = synchronous, bit for bit
    _replay(cs, method, f"{lsname}/second generation", pipelined)
    _replay(cs, method, f"{lsname}/generic", generic)


@pytest.mark.parametrize("method,lsname", METHODS)
@pytest.mark.parametrize("cs,world", E.SHARDED, ids=lambda v: repr(v) if isinstance(v, E.Case) else f"P{v}")
def test_row_sharded_runs_replay_and_every_rank_has_the_same_bits(qn, cs, world, method, lsname):
    a, c, _ = E.problem(cs.name)

    def body(rank, world_, group):
        ctx = qn.Context(0, rank=rank, world=world_, host_allgather=group.allgather_fn(rank))
        try:
            obj = qn.LogSumExp(a, c, E.MU, ctx=ctx)
            try:
                out = _solve(qn, cs, method, lsname, obj, ctx=ctx)
                group.sync()
                return out
            finally:
                obj.close()
        finally:
            ctx.close()

    res = run_ranks(world, body)
    for r in res:
        assert r[2] & 16, r[2]  # the second-generation structure, not a fallback to the generic path
        assert _same_bits(r, res[0])
    _replay(cs, method, f"{lsname}/{world} ranks", res[0])


def _hold(cs, tag, f, g):
    a, c, x0 = E.problem(cs.name)
    cache = _truths.setdefault(cs.name, {})
    if x0.tobytes() not in cache:
        cache[x0.tobytes()] = E.Truth(a, c, x0)
    rf, rg = E.point_ratios(cache[x0.tobytes()], f, g)
    print(f"lse obj(x0) {cs.name}/{tag}: ratio of f {rf:.3e}, of g {rg:.3e}")
    WORST_OBJ[cs.label] = max(WORST_OBJ.get(cs.label, 0.0), rf, rg)
    assert rf <= 1.0 and rg <= 1.0, (cs.name, tag, rf, rg)


@pytest.mark.parametrize("cs", SINGLE, ids=repr)
def test_stand_alone_evaluation_one_pass_and_two_pass(qn, cs, monkeypatch):
    a, c, x0 = E.problem(cs.name)
    one = qn.LogSumExp(a, c, E.MU)
    monkeypatch.setenv("QN_LSE_TWO_PASS", "1")
    two = qn.LogSumExp(a, c, E.MU)
    monkeypatch.delenv("QN_LSE_TWO_PASS")
    for tag, obj in (("one pass", one), ("two passes", two)):
        ev = obj(x0)
        _hold(cs, tag, ev.f(), ev.g())
        obj.close()


@pytest.mark.parametrize("cs,world", E.SHARDED, ids=lambda v: repr(v) if isinstance(v, E.Case) else f"P{v}")
def test_stand_alone_evaluation_row_sharded(qn, cs, world, monkeypatch):
    a, c, x0 = E.problem(cs.name)

    def body(rank, world_, group):
        ctx = qn.Context(0, rank=rank, world=world_, host_allgather=group.allgather_fn(rank))
        try:
            obj = qn.LogSumExp(a, c, E.MU, ctx=ctx)
            try:
                ev = obj(x0)
                out = (ev.f(), np.array(ev.g()))
                group.sync()
                return out
            finally:
                obj.close()
        finally:
            ctx.close()

    for tag, two_pass in (("one pass", False), ("two passes", True)):
        if two_pass:
            monkeypatch.setenv("QN_LSE_TWO_PASS", "1")
        res = run_ranks(world, body)
        if two_pass:
            monkeypatch.delenv("QN_LSE_TWO_PASS")
        for f, g in res:
            assert np.array_equal(f, res[0][0], equal_nan=True) and np.array_equal(g, res[0][1], equal_nan=True)
        _hold(cs, f"{tag}, {world} ranks", *res[0])


def test_skip_cap_over_everything_replayed_and_the_record_of_ratios():
    """(last in the file: the tally of the replays above.  The ratios are a record for the next reader, not a tolerance.)"""
    for fam in sorted(set(WORST) | set(WORST_OBJ)):
        print(f"lse on the GPU, {fam:18s} worst ratio of the runs' replays {WORST.get(fam, 0.0):.3e}, of obj(x0) {WORST_OBJ.get(fam, 0.0):.3e}")
    print(f"skipped {TALLY.skipped} of {TALLY.triples} (run, iteration, check) triples")
    TALLY.check()
