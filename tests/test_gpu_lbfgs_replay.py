"""Every L-BFGS direction of a GPU run (kernels csrc/qn_lbfgs.hip.h, the commit branch of vec_post_kernel) replayed in extended precision from the
run's own pairs: tests/lbfgs_replay.py, where the element-wise bound is derived; cases and conditions in lbfgs_cases.REPLAY_CASES, licensed on the
CPU by tests/test_ref_lbfgs_replay.py.  Every case runs on a host closure that records what it was asked and what it answered, so the replay
uses the gradients the device was handed.  Unlike the trajectory parity of tests/test_gpu_lbfgs.py nothing accumulates: each iteration is
predicted from the GPU's own x_k, t_k and memory, so the check runs through the whole run, with a full and wrapping ring, behind any line search.

Per case the test prints the worst ratio (asserted <= 1), the iterations asserted and skipped, the largest k and the head advances."""
import numpy as np
import pytest

import lbfgs_cases as C
import lbfgs_replay as LR
from test_ref_lbfgs_replay import check_conditions

pytestmark = pytest.mark.gpu


def _search(qn, kind, lb, ub):
    if kind == "gll":
        return qn.GLLQuadratic(1e-4, 10)
    if kind == "bt":
        return qn.BackTracking(1e-4, 0.5)
    if kind == "sw":
        return qn.StrongWolfe()
    return qn.BackTrackingB(1e-4, 0.5, lb, ub)


def gpu_run(qn, case):
    fn, x0, lb, ub = C.replay_problem(case)
    rec = LR.Recorder(fn)
    s = qn.ProjectedLBFGS(case["tol"], x0, lb, ub, m=case["m"], memoize=case["memoize"])
    if case["unit"]:
        s.set_option("lbfgs_unit_scaling", 1)
    run = LR.Run(case["m"], case["unit"], lb, ub, x0, rec)
    ls = _search(qn, case["ls"], lb, ub)
    for _ in range(case["calls"]):
        s.set_trace(case["iters"], with_x=True)
        states = []
        try:
            s.minimize(ls, rec, case["iters"], 50, callback=lambda r: states.append((r.stored_pairs(), r.gamma(), r.resets())))
        except qn.MaxIterReached:
            pass
        tr, xs = s.trace()
        run.extend(list(xs), [r["t"] for r in tr], [r["updated"] for r in tr], states)
    assert np.array_equal(s.x(), run.xs[-1])
    s.close()
    return run


@pytest.mark.parametrize("case", C.REPLAY_CASES, ids=[c["name"] for c in C.REPLAY_CASES])
def test_replay(qn, case):
    run = gpu_run(qn, case)
    rep = LR.replay(run)
    LR.check(rep, case["name"])
    check_conditions(case, rep)
    if case["box"]:
        x = run.xs[-1]
        assert 0 < int(np.sum((x == run.lb) | (x == run.ub))) < x.size  # some coordinates end on a bound, some inside the box
    if case["prob"] == "zero":
        assert rep.resets >= 1
    if case["name"] == "grid-wraps-m5":
        assert rep.max_k == 5 and rep.iterations == case["iters"]  # two Gram groups (4 + 1) at a size where the grid-stride loop wraps
    if case["calls"] > 1:
        assert rep.iterations == case["iters"] * case["calls"] and rep.head_advances > case["iters"]  # the ring went on turning across the call boundary
