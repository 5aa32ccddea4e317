"""GPU: dense quasi-Newton runs on device quadratics -- the path the benchmark times -- replayed in extended precision from their own recorded
iterates (tests/qn_replay.py, with the truth, bounds, problems and segment plans of tests/quad_replay_cases.py; licensed on the CPU by
tests/test_ref_quad_replay.py).  Per iteration f, gnorm, s_norm, y_norm and, entry by entry, the step against -t H_k g_k (in a box:
t (P(x - H_k g_k) - x)); at the end of every segment the matrix approx_inv_hessian() returns, entry by entry, and its bitwise symmetry where the path
promises it.  A run is a sequence of minimize calls on one solver; the matrix read between the calls is the next segment's start, so the bound on
the device's H never accumulates over more than three iterations, and the calls end in every state of the store-skip (one update pending, two,
a stored pass followed by one; the getter's flush of one and of two).

What is replayed: BFGS / DFP with More-Thuente and backtracking on the row kernels (n = 7, 130, 1000; chunks_per_trip 2 and 4), the
first-generation symmetric tiles (n = 1020) and the second generation (n = 1024, 1152, 4096), each option switched off at the smallest size where
it changes what runs (n = 1024: second_generation, symmetric_storage, hpass_store_skip, pipelined / synchronous; n = 4096: row_slivers,
eval_pair_instance, eval_mover_multiplier, eval_zigzag); SR1B / BFGSB / DFPB in the box of the cases file with MoreThuenteB / BackTrackingB on the
second-generation path and on the generic one at n = 1024, and on the G = 256 instantiations at n = 4096 with BackTrackingB's projection inside
the evaluation kernel and as a launch per trial; row-sharded runs on 2, 3 and
4 ranks (ranks as threads, every rank the same bits); a host closure on the generic path, whose own outputs are the truth (bg = 0: the H pass alone
under the tightest bound the method has); one non-symmetric Q (full-matrix row kernels); a problem whose entries span twelve decades; and
stand-alone obj(x0) of every problem.

n = 4096 is replayed as ONE segment of three iterations per run (from H = I: the direction pass and three update passes, the second of which
does not store): its longdouble products are n^2 each, and a second segment would take a test past a few seconds.  So at n = 4096 the start matrix
read back, the getter's flush of two pending updates and the warm continuation are NOT replayed; n = 1024 and 1152 have them.

The worst asserted ratios on an MI355X per path are printed by the last test and recorded in tests/quad_replay_cases.py's docstring (a record, not
a tolerance): 0.12 at the most (a direction of the twelve-decade problem), 0.011 for a direction on the second-generation path, 0.077 for an entry of
a stored H; nothing failed on the library as it stood.  Not replayed here: touch_h_rows / touch_q_rows, machine_fast_steps, tail_reduce and
folded_accept_reduce off their defaults, and tiles1."""
import numpy as np
import pytest

import qn_replay as R
import quad_replay_cases as Q
from thread_ranks import run_ranks

pytestmark = pytest.mark.gpu

TALLY = R.Tally()
WORST = {}       # (path label, check) -> worst asserted ratio
WORST_OBJ = {}   # problem -> worst ratio of obj(x0)
LS_ITERS = 100   # (the wide problem's first step is 1e-12: forty halvings)
FREE = [("bfgs", "mt"), ("bfgs", "bt"), ("dfp", "mt"), ("dfp", "bt")]
TWO = [("bfgs", "mt"), ("dfp", "bt")]
NPAD = {7: 16, 130: 144, 1000: 1008, 1020: 1024, 1024: 1024, 1152: 1152, 4096: 4096}
_objs = {}


def sym_bytes(n):
    """bytes one pass of the second-generation path streams (tests/test_gpu_symmetric.py)"""
    nb = n // 128
    return nb * (nb - 1) // 2 * 128 * 128 * 8 + nb * 73728


@pytest.fixture(scope="module", autouse=True)
def _close_objectives():
    yield
    for obj in _objs.values():
        obj.close()
    _objs.clear()


def _obj(qn, kind, n):
    if (kind, n) not in _objs:
        q, b, _ = Q.problem(kind, n)
        _objs[(kind, n)] = qn.Quadratic(q, b)
    return _objs[(kind, n)]


def _ls(qn, lsname, n=None, bx=None):
    if lsname == "mt":
        return qn.MoreThuente()
    if lsname == "bt":
        return qn.BackTracking(1e-4, 0.5)
    if lsname == "mtb":
        return qn.MoreThuenteB.new(n).with_lower_bound(bx[0]).with_upper_bound(bx[1])
    return qn.BackTrackingB.new(1e-4, 0.5, bx[0], bx[1])


class Runner:
    """one solver driven call by call (quad_replay_cases.run_plan)"""

    def __init__(self, qn, method, lsname, oracle, x0, total, bx=None, options=(), sync=None, ctx=None, all_ranks=False, memoize=None):
        self.qn, self.oracle, self.all_ranks = qn, oracle, all_ranks
        kw = {"ctx": ctx} if ctx is not None else {}
        if bx is None:
            self.s = {"bfgs": qn.BFGS, "dfp": qn.DFP, "broyden": qn.Broyden}[method](1e-10, x0, **kw)
        else:
            self.s = {"bfgs": qn.BFGSB, "dfp": qn.DFPB, "sr1": qn.SR1B, "broyden": qn.BroydenB}[method].new(1e-10, x0, bx[0], bx[1])
        if memoize is not None:  # (None: the solver's default for the oracle's kind)
            self.s.memoize = memoize
        self.s.set_trace(total, with_x=True)
        for name, v in options:
            self.s.configure(name, v)
        if sync is not None:
            self.s.set_sync_mode(sync)
        self.ls = _ls(qn, lsname, x0.size, bx)
        self.tr, self.xs = [], []

    def advance(self, iters):
        """one minimize call (k and the trace start again with every call, ls_solver.rs:74-76: the records are collected here)"""
        try:
            self.s.minimize(self.ls, self.oracle, iters, LS_ITERS)
        except self.qn.MaxIterReached:
            pass
        tr, xs = self.s.trace()
        assert len(tr) == iters, ("the call ended early", len(tr), iters)
        self.tr += tr
        self.xs += [np.array(x) for x in xs]

    def records(self):
        return list(self.tr), np.array(self.xs)

    def inv_hessian(self):
        return self.s.approx_inv_hessian(all_ranks=True) if self.all_ranks else self.s.approx_inv_hessian()

    def close(self):
        self.s.close()


def _hold(label, name, truth, method, segs, bx=None, symmetric=False):
    reps = Q.replay_plan(name, truth, method, segs, box=bx, symmetric=symmetric)
    for rep in reps:
        R.check(rep)
        for c in R.CHECKS + ("H",):
            WORST[(label, c)] = max(WORST.get((label, c), 0.0), rep.worst_of(c))
    TALLY.add_run(reps)


def _run(qn, kind, n, method, lsname, plan, read_h, boxed=False, options=(), sync=None):
    """-> (segments, stats of the last call, box)"""
    x0 = Q.problem(kind, n)[2]
    bx = Q.box(x0) if boxed else None
    rn = Runner(qn, method, lsname, _obj(qn, kind, n), x0, sum(plan), bx, options, sync)
    try:
        segs = Q.run_plan(rn, x0 if bx is None else np.clip(x0, bx[0], bx[1]), plan, read_h)
        return segs, rn.s.stats(), bx
    finally:
        rn.close()


def _plans(n):
    if n == 4096:  # (its longdouble products are n^2 each: one segment of three)
        return [((3,), True)]
    return [(p, True) for p in Q.PLANS] + [(p, False) for p in Q.WARM_PLANS]


def _plan_id(v):
    return "+".join(map(str, v[0])) + ("" if v[1] else "warm")


FREE_CASES = [(n, m, l, pl) for n in Q.SIZES for (m, l) in (FREE if n < 4096 else TWO) for pl in _plans(n)]


@pytest.mark.parametrize("n,method,lsname,plan", FREE_CASES, ids=lambda v: _plan_id(v) if isinstance(v, tuple) else str(v))
def test_bfgs_and_dfp_on_every_size(qn, n, method, lsname, plan):
    segs, st, _ = _run(qn, "synth", n, method, lsname, plan[0], plan[1])
    rpr, n_pad = qn.partition(n, 1)
    assert n_pad == NPAD[n]
    if n < 1020:
        assert st["path"] & 1 and not st["path"] & 2 and st["matrix_bytes_per_pass"] == rpr * n_pad * 8, st["path"]
        label = f"row kernels n={n}"
    elif n == 1020:
        assert st["path"] & 2 and not st["path"] & 16 and st["matrix_bytes_per_pass"] == 36 * 128 * 128 * 8, st["path"]
        label = "first-generation tiles n=1020"
    else:
        assert st["path"] & 16 and st["matrix_bytes_per_pass"] == sym_bytes(n), st["path"]
        label = f"second generation n={n}"
    _hold(label, f"synth{n}/{method}/{lsname}/{_plan_id(plan)}", Q.truth_factory("synth", n), method, segs, symmetric=bool(st["path"] & 2))


@pytest.mark.parametrize("method,lsname", TWO)
@pytest.mark.parametrize("chunks", [2, 4])
def test_row_kernels_with_more_chunks_per_trip(qn, chunks, method, lsname):
    """(qn_option's text promises nothing about the bits against one chunk per trip: each variant is held to the bounds)"""
    segs, st, _ = _run(qn, "synth", 1000, method, lsname, (3, 3), True, options=(("chunks_per_trip", chunks),))
    assert st["path"] & 1 and not st["path"] & 2
    _hold(f"row kernels n=1000, {chunks} chunks per trip", f"synth1000/{method}/{lsname}/chunks{chunks}", Q.truth_factory("synth", 1000), method, segs)


# (row_slivers, eval_pair_instance, eval_mover_multiplier and btb_project_in_eval change nothing at nb = 8: see the n = 4096 tests below)
VARIANTS = [("second_generation", 0), ("symmetric_storage", 0), ("hpass_store_skip", 0), ("hpass_store_skip", 1), ("pipelined", None),
            ("synchronous", None)]


@pytest.mark.parametrize("method,lsname", TWO)
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}={v[1]}")
def test_second_generation_variants_at_1024(qn, variant, method, lsname):
    n = 1024
    opts = () if variant[1] is None else (variant,)
    sync = {"pipelined": 0, "synchronous": 1}.get(variant[0])
    for plan in ((1, 2, 3), (2, 2, 2)):
        segs, st, _ = _run(qn, "synth", n, method, lsname, plan, True, options=opts, sync=sync)
        p = st["path"]
        if variant == ("second_generation", 0):
            assert p & 2 and not p & 16, p
        elif variant == ("symmetric_storage", 0):
            assert p & 1 and not p & 2 and st["matrix_bytes_per_pass"] == n * n * 8, p
        else:
            assert p & 16 and st["matrix_bytes_per_pass"] == sym_bytes(n), p
        if variant[0] == "pipelined":
            assert p & 8
        if variant[0] == "synchronous":
            assert not p & 8
        if variant == ("hpass_store_skip", 0):
            assert st["n_hpass_nostore"] == 0
        _hold(f"n=1024 {variant[0]}={variant[1]}", f"synth{n}/{method}/{lsname}/{variant[0]}={variant[1]}/{_plan_id((plan, True))}",
              Q.truth_factory("synth", n), method, segs, symmetric=bool(p & 2))


def test_store_skip_states_are_reached(qn):
    """the plans end their calls where the cases file says: (2, 2, 2) leaves two updates pending after every call (each call's second update pass
    does not store), (3, 3) one read pass per call"""
    for plan, nostore in (((2, 2, 2), 1), ((3, 3), 1), ((1, 2, 3), None)):
        x0 = Q.problem("synth", 1024)[2]
        rn = Runner(qn, "bfgs", "mt", _obj(qn, "synth", 1024), x0, sum(plan))
        try:
            seen = []
            for iters in plan:
                rn.advance(iters)
                seen.append(rn.s.stats()["n_hpass_nostore"])
                rn.inv_hessian()
        finally:
            rn.close()
        print("read passes per call of", plan, seen)
        if nostore is not None:
            assert seen == [nostore] * len(plan), (plan, seen)
        else:
            assert seen == [0, 1, 1], seen


# THE G = 256 INSTANTIATIONS exist from n = 4096 on only.  solver_alloc_sym2 (qn_host_solver.hip.h) deals nb (nb + 1) / 2 items to G = min(items, 256)
# workgroups: nb = 8 gives 36 workgroups of one item and no slivers (L = 0, sl_per = 0), and plan_s2_args (qn_host_minimize.hip.h) then has
# pair = 0, hence ring = 0, hence projfold = 0 whatever the options say.  nb = 32 gives 528 items, G = 256, L = 16 slivers, two items per workgroup:
# the pair instance, its mover / multiplier form (s2_evalr_kernel, zig-zag, touch workgroups) and BackTrackingB's projection inside it.  So the options
# that switch those off, and the bounded / SR1 instantiations of those kernels, are replayed here, one segment of three iterations each.  (No counter
# says which instance ran, except the launches the in-kernel projection saves; the conditions above are read from the code.)
@pytest.mark.parametrize("option", ["row_slivers", "eval_pair_instance", "eval_mover_multiplier", "eval_zigzag"])
def test_second_generation_fallbacks_at_4096(qn, option):
    n = 4096
    segs, st, _ = _run(qn, "synth", n, "bfgs", "mt", (3,), True, options=((option, 0),))
    assert st["path"] & 16 and st["matrix_bytes_per_pass"] == sym_bytes(n), st["path"]
    _hold(f"n=4096 {option}=0", f"synth{n}/bfgs/mt/{option}=0/3", Q.truth_factory("synth", n), "bfgs", segs, symmetric=True)


_launches = {}


@pytest.mark.parametrize("method,lsname,proj", [("bfgs", "btb", 1), ("bfgs", "btb", 0), ("sr1", "mtb", 1), ("dfp", "mtb", 1), ("sr1", "btb", 1)])
def test_bounded_solvers_in_the_box_at_4096(qn, method, lsname, proj):
    """the bounded and SR1 instantiations of the G = 256 kernels (s2_dir at G = 256, s2_eval / s2_evalr with BND) and BackTrackingB's trial points
    projected inside the mover / multiplier kernel (proj = 1, the default) or by a launch per trial (proj = 0)"""
    n = 4096
    segs, st, bx = _run(qn, "synth", n, method, lsname, (3,), True, boxed=True, options=(("btb_project_in_eval", proj),))
    assert st["path"] & 16, st["path"]
    for sg in segs:
        assert np.all(sg["xs"] >= bx[0] - 1e-12) and np.all(sg["xs"] <= bx[1] + 1e-12)
    if (method, lsname) == ("bfgs", "btb"):  # the in-kernel projection did run: at least one launch per evaluation fewer than with a launch per trial
        _launches[proj] = (st["launches"], st["oracle_evals"])
        if len(_launches) == 2:
            assert _launches[1][1] == _launches[0][1] and _launches[0][0] - _launches[1][0] >= _launches[1][1], _launches
    _hold(f"box n=4096 {lsname}", f"box{n}/{method}/{lsname}/proj={proj}/3", Q.truth_factory("synth", n), method, segs, bx=bx, symmetric=True)


BOXED = [(m, l, s2) for m in ("sr1", "bfgs", "dfp") for l in ("mtb", "btb") for s2 in (1, 0)]


@pytest.mark.parametrize("method,lsname,s2", BOXED)
def test_bounded_solvers_in_the_box_at_1024(qn, method, lsname, s2):
    n = 1024
    opts = (("bounded_second_generation", s2),)
    for plan, read_h in (((3, 3), True), ((1, 2, 3), True), ((6,), False)):
        segs, st, bx = _run(qn, "synth", n, method, lsname, plan, read_h, boxed=True, options=opts)
        assert bool(st["path"] & 16) == bool(s2), st["path"]
        if not s2:
            assert st["path"] & 4, st["path"]  # the generic path, its H pass on the symmetric tiles
        for sg in segs:  # every iterate inside the box (to rounding)
            assert np.all(sg["xs"] >= bx[0] - 1e-12) and np.all(sg["xs"] <= bx[1] + 1e-12)
        _hold(f"box n=1024 {'second generation' if s2 else 'generic'}", f"box{n}/{method}/{lsname}/s2={s2}/{_plan_id((plan, read_h))}",
              Q.truth_factory("synth", n), method, segs, bx=bx, symmetric=True)


SHARDED = [(1024, 2), (1024, 4), (1152, 3), (1000, 2)]


@pytest.mark.parametrize("method,lsname", TWO)
@pytest.mark.parametrize("n,world", SHARDED, ids=lambda v: str(v))
def test_row_sharded_runs_and_every_rank_has_the_same_bits(qn, n, world, method, lsname):
    q, b, x0 = Q.problem("synth", n)
    for plan, read_h in (((3, 3), True), ((6,), False)):
        def body(rank, world_, group):
            ctx = qn.Context(0, rank=rank, world=world_, host_allgather=group.allgather_fn(rank))
            try:
                obj = qn.Quadratic(q, b, ctx=ctx)
                try:
                    rn = Runner(qn, method, lsname, obj, x0, sum(plan), ctx=ctx, all_ranks=True)
                    try:
                        segs = Q.run_plan(rn, x0, plan, read_h)
                        out = (segs, rn.s.stats()["path"])
                        group.sync()
                        return out
                    finally:
                        rn.close()
                finally:
                    obj.close()
            finally:
                ctx.close()

        res = run_ranks(world, body, timeout=120.0)
        for segs, path in res:
            assert path & 2 and bool(path & 16) == (n != 1000), path  # (n = 1000: rpr = 512, n_pad = 1024: first-generation sharded tiles with padding)
            for a, c in zip(segs, res[0][0]):
                assert a["tr"] == c["tr"] and np.array_equal(a["xs"], c["xs"]) and np.array_equal(a["h_end"], c["h_end"])
        _hold(f"{world} ranks n={n}", f"synth{n}/{method}/{lsname}/{world} ranks/{_plan_id((plan, read_h))}", Q.truth_factory("synth", n), method,
              res[0][0], symmetric=True)


@pytest.mark.parametrize("method,lsname", TWO)
@pytest.mark.parametrize("n", [1020, 1024])
def test_host_closure_on_the_generic_path(qn, n, method, lsname):
    """the closure's own float64 outputs are the truth (bf = bg = 0): y is exact up to one subtraction, and the generic path's H pass on the
    symmetric tiles stands alone under the bound"""
    q, b, x0 = Q.problem("synth", n)
    seen = {}

    def fn(x):
        qx = q @ x
        out = (0.5 * float(x @ qx) - float(b @ x), qx - b)
        seen[x.tobytes()] = out
        return out

    def truth(x):
        if x.tobytes() not in seen:
            fn(np.array(x))
        return Q.ClosureTruth(*seen[x.tobytes()])

    for plan, read_h in (((3, 3), True), ((1, 2, 3), True)):
        rn = Runner(qn, method, lsname, fn, x0, sum(plan))
        try:
            segs = Q.run_plan(rn, x0, plan, read_h)
            path = rn.s.stats()["path"]
        finally:
            rn.close()
        assert path & 4 and not path & 1, path
        _hold(f"closure n={n}", f"closure{n}/{method}/{lsname}/{_plan_id((plan, read_h))}", truth, method, segs, symmetric=True)


@pytest.mark.parametrize("method,lsname", TWO)
def test_a_non_symmetric_q_takes_the_full_matrix_row_kernels(qn, method, lsname):
    n = 1024
    for plan, read_h in (((3, 3), True), ((6,), False)):
        segs, st, _ = _run(qn, "nonsym", n, method, lsname, plan, read_h)
        assert st["path"] & 1 and not st["path"] & 2 and st["matrix_bytes_per_pass"] == n * n * 8, st["path"]
        _hold("non-symmetric Q n=1024", f"nonsym{n}/{method}/{lsname}/{_plan_id((plan, read_h))}", Q.truth_factory("nonsym", n), method, segs)


@pytest.mark.parametrize("method,lsname", TWO)
@pytest.mark.parametrize("n", [130, 1024])
def test_entries_spanning_twelve_decades(qn, n, method, lsname):
    for plan, read_h in (((3, 3), True), ((6,), False)):
        segs, st, _ = _run(qn, "wide", n, method, lsname, plan, read_h)
        assert bool(st["path"] & 16) == (n == 1024)
        _hold(f"wide n={n}", f"wide{n}/{method}/{lsname}/{_plan_id((plan, read_h))}", Q.truth_factory("wide", n), method, segs, symmetric=bool(st["path"] & 2))


OBJ_CASES = [("synth", n) for n in Q.SIZES] + [("wide", 130), ("wide", 1024), ("nonsym", 1024)]


@pytest.mark.parametrize("kind,n", OBJ_CASES)
def test_stand_alone_evaluation(qn, kind, n):
    x0 = Q.problem(kind, n)[2]
    ev = _obj(qn, kind, n)(x0)
    rf, rg = R.point_ratios(Q.truth_factory(kind, n)(x0), ev.f(), ev.g())
    print(f"quad obj(x0) {kind}{n}: ratio of f {rf:.3e}, of g {rg:.3e}")
    WORST_OBJ[kind] = max(WORST_OBJ.get(kind, 0.0), rf, rg)
    assert rf <= 1.0 and rg <= 1.0, (kind, n, rf, rg)


def test_skip_caps_and_the_record_of_ratios():
    """(last in the file: the tally of the replays above.  The ratios are a record for the next reader, not a tolerance.)"""
    labels = sorted({k[0] for k in WORST})
    for lab in labels:
        per = ", ".join(f"{c} {WORST.get((lab, c), 0.0):.2e}" for c in R.CHECKS + ("H",))
        print(f"quad on the GPU, {lab:42s} worst ratios: {per}")
    for kind, r in sorted(WORST_OBJ.items()):
        print(f"quad on the GPU, obj(x0) {kind:7s} worst ratio {r:.3e}")
    print(f"skipped {TALLY.skipped} of {TALLY.triples} (run, iteration, check) triples")
    assert TALLY.triples > 0, "this test reports on the replays of the tests in front of it: run the file, not this test alone"
    TALLY.check()
