"""GPU: Broyden / BroydenB runs on device quadratics replayed in extended precision from their own recorded iterates (tests/qn_replay.py, method
"broyden"; cases, sizes and the restatement's licence: tests/broyden_replay_cases.py, tests/test_ref_broyden_replay.py).  Per iteration f, gnorm,
s_norm, y_norm and, entry by entry, the step against -t H_k g_k (in a box: t (P(x - H_k g_k) - x)); at the end of every segment the matrix
approx_inv_hessian() returns, entry by entry, and that it is clearly NOT symmetric.

What runs: r1_pass_kernel's instances 4, 5, 6 (memoize = 0), 4, 9, 11 and the control step's lazy direction (memoize = 1), 2 (the getter between
the calls of a plan), and 6 at a call's entry (the warm plans), at n = 7, 128, 129, 257, 384 and 1024.  Every case asserts from stats() that the run
took QN_PATH_RANK1 and none of the symmetric paths, and the number of passes over H and their bytes, so that a case silently routed elsewhere fails.
The worst asserted ratios are printed by the last test and recorded in tests/broyden_replay_cases.py's docstring (a record, not a tolerance)."""
import numpy as np
import pytest

import broyden_replay_cases as B
import qn_replay as R
import quad_replay_cases as Q
from test_gpu_quad_replay import Runner  # (drives one solver call by call)

pytestmark = pytest.mark.gpu

TALLY = R.Tally()
WORST = {}   # (n, check) -> worst asserted ratio
_objs = {}


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


class _Counted(Runner):
    """the Runner, with what every call of a plan must have cost asserted as it goes"""

    def __init__(self, qn, n, *args, **kw):
        super().__init__(qn, "broyden", *args, **kw)
        self.n, self.memo, self.entered_pending = n, kw["memoize"], 0

    def advance(self, iters):
        done = len(self.tr)
        super().advance(iters)
        st, abi = self.s.stats(), self.qn._abi
        assert all(r["updated"] for r in self.tr[done:]), "an iteration without an update: the plan does not fit this case"
        assert st["path"] & abi.PATH_RANK1, st["path"]
        assert not st["path"] & (abi.PATH_FUSED | abi.PATH_SYM | abi.PATH_SYM_GENERIC | abi.PATH_SYM2 | abi.PATH_PIPELINED), st["path"]
        # a call opens with a direction pass; memoize = 1: then ONE pass per iteration, memoize = 0: two.  Passes that found an update pending and
        # wrote H back: every iteration's but the first, and the opening pass of a call entered with one (no getter in front of it)
        n_pad = B.NPAD[self.n]
        assert st["h_passes"] == (iters + 1 if self.memo else 2 * iters), (st["h_passes"], iters, self.memo)
        assert st["h_bytes"] == (st["h_passes"] + iters - 1 + self.entered_pending) * n_pad * n_pad * 8, (st["h_bytes"], iters, self.entered_pending)
        self.entered_pending = 1

    def inv_hessian(self):
        self.entered_pending = 0  # the getter flushes
        return super().inv_hessian()


def _run(qn, kind, n, lsname, boxed, memoize, plan, read_h):
    x0 = Q.problem(kind, n)[2]
    bx = Q.box(x0) if boxed else None
    assert qn.partition(n, 1)[1] == B.NPAD[n]
    rn = _Counted(qn, n, lsname, _obj(qn, kind, n), x0, sum(plan), bx, memoize=memoize)
    try:
        return Q.run_plan(rn, x0 if bx is None else np.clip(x0, bx[0], bx[1]), plan, read_h), bx
    finally:
        rn.close()


def _hold(n, name, truth, segs, bx=None):
    reps = Q.replay_plan(name, truth, "broyden", segs, box=bx)
    for rep, sg in zip(reps, segs):
        R.check(rep)
        for c in R.CHECKS + ("H",):
            WORST[(n, c)] = max(WORST.get((n, c), 0.0), rep.worst_of(c))
        asym = B.asymmetry(sg["h_end"])
        assert asym > B.NOT_SYMMETRIC * rep.dh_max, (rep.name, "the matrix read back is not clearly non-symmetric", asym, rep.dh_max)
    TALLY.add_run(reps)


def _id(v):
    return B.plan_id(v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("kind,n,lsname,boxed,memoize,plan", B.GPU_CASES, ids=_id)
def test_replay(qn, kind, n, lsname, boxed, memoize, plan):
    segs, bx = _run(qn, kind, n, lsname, boxed, memoize, plan[0], plan[1])
    if bx is not None:  # every iterate inside the box (to rounding)
        for sg in segs:
            assert np.all(sg["xs"] >= bx[0] - 1e-12) and np.all(sg["xs"] <= bx[1] + 1e-12)
    _hold(n, f"{kind}{n}/broyden/{lsname}/memoize={memoize}/{B.plan_id(plan)}", Q.truth_factory(kind, n), segs, bx=bx)


# one case per instance family: memoize = 0 (4, 5, 6), memoize = 1 (4, 9, 11, the lazy direction), the warm entry (6 at a call's start), the box
SAME_BITS = [("synth", 257, "mt", False, 0, ((3, 3), True)), ("synth", 257, "bt", False, 1, ((1, 2, 3), True)),
             ("synth", 129, "mt", False, 1, ((3, 3), False)), ("synth", 129, "btb", True, 1, ((3, 3), True))]


@pytest.mark.parametrize("kind,n,lsname,boxed,memoize,plan", SAME_BITS, ids=_id)
def test_two_identical_runs_give_the_same_bits(qn, kind, n, lsname, boxed, memoize, plan):
    one, two = (_run(qn, kind, n, lsname, boxed, memoize, plan[0], plan[1])[0] for _ in range(2))
    assert len(one) == len(two)
    for a, c in zip(one, two):
        assert a["tr"] == c["tr"] and np.array_equal(a["xs"], c["xs"]) and np.array_equal(a["h_end"], c["h_end"])


def test_skip_caps_and_the_record_of_ratios():
    """(last in the file: the tally of the replays above.  The ratios are a record for the next reader, not a tolerance.)"""
    for n in sorted({k[0] for k in WORST}):
        print(f"broyden on the GPU, n = {n:5d} worst ratios: " + ", ".join(f"{c} {WORST.get((n, c), 0.0):.2e}" for c in R.CHECKS + ("H",)))
    print(f"skipped {TALLY.skipped} of {TALLY.triples} (run, iteration, check) triples; the seeded matrix is the {Q.SOURCE.get('synth')}'s")
    assert TALLY.triples > 0, "this test reports on the replays of the tests in front of it: run the file, not this test alone"
    TALLY.check()
