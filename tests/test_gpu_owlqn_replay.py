"""Every iteration of GPU OWLQN runs on host closures replayed in extended precision from the run's own pairs: tests/owlqn_replay.py (lbfgs_replay's
Memory and Direction applied to the pseudo-gradient, then rules 3 and 5 entry by entry, an entry whose alignment or orthant decision the bound cannot
decide accepted at either outcome).  Cases and problems: owlqn_cases.REPLAY_CASES, licensed on the CPU by
tests/test_ref_owlqn.py::test_replay_is_licensed_on_the_restatement.  Nothing accumulates from one iteration to the next, so the check runs through
whole runs with the ring full and wrapping, and across a call boundary.

Per case the test prints the worst ratio (asserted <= 1), the iterations asserted and skipped, the largest k, the head advances and the undecided
entries; the conditions (at most a fifth skipped, at most 1 % undecided) are owlqn_replay.check_conditions."""
import numpy as np
import pytest

import owlqn_cases as C
import owlqn_replay as OR

pytestmark = pytest.mark.gpu


def gpu_run(qn, case):
    fn, x0, l1 = C.replay_problem(case)
    rec = OR.Recorder(fn)
    s = qn.OWLQN(C.REPLAY_TOL, x0, l1, m=case["m"])
    run = OR.Run(case["m"], False, l1, x0, rec)
    ls = qn.BackTracking(C.C1, C.BETA)
    for _ in range(case["calls"]):
        s.set_trace(case["iters"], with_x=True)
        states = []
        try:
            s.minimize(ls, rec, case["iters"], C.MAX_LS, callback=lambda r: states.append((r.stored_pairs(), r.gamma(), r.resets())))
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
    rep = OR.replay(run)
    OR.check(rep, case["name"])
    assert rep.iterations == case["iters"] * case["calls"]
    assert rep.commits > case["m"] and rep.head_advances > 0  # the ring wraps
    if case["m"] == 32:
        assert rep.max_k == 32
    if case["calls"] > 1:
        assert rep.head_advances > case["iters"]  # the ring went on turning across the call boundary
    assert 0 < np.count_nonzero(run.xs[-1]) < case["n"]
