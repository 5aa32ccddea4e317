"""CPU: licenses tests/qn_replay.py with the truth and bounds of tests/quad_replay_cases.py, the checker tests/test_gpu_quad_replay.py holds the
device to.  A float64 restatement of BFGS / DFP / SR1 on the quadratic (free and in the box, continued over several calls, its matrix read between
them) must replay with every ratio <= 1 and within the skip caps in three summation orders -- numpy's, every sum reversed, and the 128-tile order
that adds mirrored off-diagonal contributions the way the symmetric half does -- and each of ten planted faults must be rejected: a checker that
accepts them would prove nothing.  Nothing here is measured against the library.

(Up to n = 130 every plan runs in all three orders.  From n = 1000 on plan (3, 3) does, and the other plans run in the tile order: the orders move
the evaluation's and the H pass's rounding, which every iteration of (3, 3) already shows at that size, while the plans only move where a segment
starts -- the same arithmetic of the checker, shown in all orders at the small sizes.  n = 4096, whose longdouble products take seconds, runs one
segment of three in one order per method (BFGS, DFP free; SR1 in the box).)"""
import numpy as np
import pytest

import qn_replay as R
import quad_replay_cases as Q

TALLY, WORST = R.Tally(), {}

# (kind, n, method, boxed)
RUNS = [("synth", n, m, False) for n in Q.SIZES if n < 4096 for m in ("bfgs", "dfp")]
RUNS += [("nonsym", 1024, "bfgs", False), ("nonsym", 130, "dfp", False)]
RUNS += [("wide", n, m, False) for n in (130, 1024) for m in ("bfgs", "dfp")]
RUNS += [("synth", n, m, True) for n in (130, 1024) for m in ("bfgs", "dfp", "sr1")]


def _run(kind, n, method, boxed, plan, read_h, order, fault=None):
    q, b, x0 = Q.problem(kind, n)
    bx = Q.box(x0) if boxed else None
    rs = Q.RefSolver(q, b, x0, method, order, box=bx, fault=fault)
    segs = Q.run_plan(rs, rs.start(), plan, read_h)
    tag = f"{kind}{n}/{method}{'/box' if boxed else ''}/{'+'.join(map(str, plan))}{'' if read_h else ' warm'}/{order}"
    return Q.replay_plan(tag, Q.truth_factory(kind, n), method, segs, box=bx, symmetric=True)


def _hold(reps, key):
    for rep in reps:
        R.check(rep)
        WORST[key] = max(WORST.get(key, 0.0), rep.worst)
    TALLY.add_run(reps)


def test_the_box_clips_a_quarter_below_a_quarter_above_and_leaves_a_quarter_free():
    for n in (7, 130, 1024):
        x0 = Q.problem("synth", n)[2]
        lb, ub = Q.box(x0)
        below, above, free = x0 < lb, x0 > ub, (x0 > lb) & (x0 < ub) & np.isfinite(lb) & np.isfinite(ub)
        assert min(below.sum(), above.sum(), free.sum()) >= n // 4 and np.all(lb < ub)
        assert np.isinf(lb).sum() >= n // 4 - 1  # (and the rest has no bounds at all: the finite-bound term of the half-width is not everywhere)


def test_the_problems_are_what_the_cases_say():
    q = Q.problem("wide", 1024)[0]
    mag = np.abs(q[q != 0])
    assert mag.min() < 1e-6 * 1e-1 and mag.max() > 1e6 * 1e-1 and np.array_equal(q, q.T)
    qn_ = Q.problem("nonsym", 1024)[0]
    assert not np.array_equal(qn_, qn_.T)
    # |Q||x| dominates |Qx| somewhere: a row whose sum cancels to less than a hundredth of its magnitudes
    _, b, x0 = Q.problem("wide", 1024)
    assert np.min(np.abs(q @ x0) / (np.abs(q) @ np.abs(x0))) < 1e-2


@pytest.mark.parametrize("kind,n,method,boxed", RUNS, ids=lambda v: str(v))
def test_three_orders_inside_the_bounds(kind, n, method, boxed):
    for order in Q.ORDERS:
        _hold(_run(kind, n, method, boxed, (3, 3), True, order), (kind, order))
    for order in (Q.ORDERS if n <= 130 else ("blocked",)):
        for plan in Q.PLANS[1:]:
            _hold(_run(kind, n, method, boxed, plan, True, order), (kind, order))
        for plan in Q.WARM_PLANS:
            _hold(_run(kind, n, method, boxed, plan, False, order), (kind, order))


@pytest.mark.parametrize("method,order,boxed", [("bfgs", "blocked", False), ("dfp", "reversed", False), ("sr1", "plain", True)])
def test_three_iterations_at_the_largest_size(method, order, boxed):
    _hold(_run("synth", 4096, method, boxed, (3,), True, order), ("synth", order))


def test_skip_caps_and_the_record_of_ratios():
    """(behind the replays above: their tally)"""
    for (kind, order), r in sorted(WORST.items()):
        print(f"quad replay of the float64 runs, {kind:7s} {order:9s} worst ratio {r:.3e}")
    print(f"skipped {TALLY.skipped} of {TALLY.triples} (run, iteration, check) triples; the seeded matrix is the {Q.SOURCE.get('synth')}'s")
    assert TALLY.triples > 0
    TALLY.check()


# ---- planted faults ----
def _rejected(reps):
    return sorted({(i, k, c) for i, rep in enumerate(reps) for k, c, r, a in rep.rows if a and not r <= 1.0})


_clean = {}


def _plant(tag, fault, kind="synth", n=130, method="bfgs", boxed=False, order="blocked", plan=(3, 3)):
    key = (kind, n, method, boxed, order, plan)
    if key not in _clean:
        _clean[key] = _rejected(_run(kind, n, method, boxed, plan, True, order))
    assert not _clean[key], (tag, "the clean run must pass")
    bad = _rejected(_run(kind, n, method, boxed, plan, True, order, fault=fault))
    print(f"planted fault {tag} on {kind}{n}/{method}: rejected (segment, iteration, check) {bad[:8]}")
    assert bad, (tag, "accepted")
    return bad


@pytest.mark.parametrize("n", [7, 130, 1024])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5])
def test_fault_1_a_gradient_entry_off_by_1e_9(n, k):
    bad = _plant(f"1 (iteration {k})", ("g_entry", k, 1e-9), n=n)
    assert (k // 3, k % 3, "dir") in bad  # ... by the direction check of that very iteration


@pytest.mark.parametrize("k", [0, 1, 2])
def test_fault_2_one_product_missing_at_the_accepted_point(k):
    n = 130
    _plant(f"2 (iteration {k})", ("drop_product", n - 1, n - 2, k), n=n)
    # the wide problem: the smallest product of the ragged tile's rows that is still a hundred times the bound of its row at x0
    q, b, x0 = Q.problem("wide", n)
    tr = Q.truth_factory("wide", n)(x0)
    prod = np.abs(q[128:] * x0[None, :])
    prod[np.arange(n - 128), np.arange(128, n)] = np.inf
    prod[prod < 100.0 * tr.bg[128:, None]] = np.inf
    i, j = np.unravel_index(np.argmin(prod), prod.shape)
    assert np.isfinite(prod[i, j])
    print(f"wide{n}: dropping Q[{128 + i},{j}] x[{j}] = {prod[i, j]:.3e}, (|Q||x|)_i = {float(np.abs(q[128 + i]) @ np.abs(x0)):.3e}")
    _plant(f"2 wide (iteration {k})", ("drop_product", 128 + int(i), int(j), k), kind="wide", n=n)


def test_fault_3_one_mirrored_contribution_missing():
    _plant("3", ("mirror", 5, 129))
    _plant("3 (n = 1024)", ("mirror", 5, 1023), n=1024)


def test_fault_4_f_off_by_1e_12():
    bad = _plant("4", ("f_off", 1e-12))
    assert {c for _, _, c in bad} == {"f"}


@pytest.mark.parametrize("k", [0, 1, 2])
def test_fault_5_one_entry_of_h_not_updated(k):
    bad = _plant(f"5 (update {k})", ("h_entry", k, 129, 128), method="dfp")
    assert (0, 2, "H") in bad and not [x for x in bad if x[0] == 0 and x[1] <= k and x[2] != "H"]  # only H and later directions can see it


def test_fault_6_one_lower_triangle_entry_not_mirrored():
    bad = _plant("6", ("no_mirror", 129, 3))
    # (the restatement goes on from its own H, not from the matrix it returned: the next segment's directions see the difference too)
    assert [x for x in bad if x[0] == 0] == [(0, 2, "H")]


def test_fault_7_the_second_pending_update_dropped_from_the_direction():
    bad = _plant("7", ("stale_dir", 2))
    assert bad[0] == (0, 2, "dir")


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("method", ["bfgs", "dfp"])
def test_fault_8_a_coefficient_from_the_previous_y_u(method, k):
    bad = _plant(f"8 (update {k})", ("stale_yu", k), method=method)
    assert (0, 2, "H") in bad


def test_fault_9_the_projection_applied_to_minus_h_g():
    _plant("9", ("project_dir",), boxed=True)


def test_fault_10_sr1_denominator_without_y_u():
    _plant("10", ("sr1_den",), method="sr1", boxed=True)


def test_detection_thresholds_of_a_wrong_gradient_entry():
    """(a record, printed: the smallest relative error still rejected, half decades at n = 7 and 130, decades at n = 1000 and 1024; the assertion is
    the fixed 1e-9 of test_fault_1)"""
    for n, step in ((7, 0.5), (130, 0.5), (1000, 1.0), (1024, 1.0)):
        for k in (0, 1, 2):
            e, last = 9.0, None
            while e <= 16.0:
                rel = 10.0 ** -e
                if not _rejected(_run("synth", n, "bfgs", False, (3,), True, "blocked", fault=("g_entry", k, rel))):
                    break
                last, e = rel, e + step
            print(f"detection threshold n = {n}, iteration {k}: smallest rejected {last:.1e}")
            assert last is not None
