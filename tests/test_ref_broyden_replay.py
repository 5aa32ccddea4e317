"""CPU: licenses tests/qn_replay.py's method "broyden" before any GPU run, on the cases of tests/broyden_replay_cases.py.  For every case the GPU
file runs, the float64 restatement (BroydenRef, with and without the lazy direction) in three summation orders must sit inside every bound with NO
triple skipped -- stricter than the tally's 10 % -- and the matrix it returns must be clearly not symmetric; each of the seven planted faults must
fail an asserted check at n = 7, 129 and 257; a gradient entry off by 1e-9 must be rejected in iterations 0 .. 2 of both segments of plan (3, 3);
and the blocked order (the kernel's tiles) must agree with the plain one far inside the bounds.  Nothing here is measured against the library."""
import numpy as np
import pytest

import broyden_replay_cases as B
import qn_replay as R
import quad_replay_cases as Q

TALLY, WORST = R.Tally(), {}


def _hold(reps, segs, n):
    for rep, sg in zip(reps, segs):
        R.check(rep)
        assert not rep.skipped, (rep.name, "skipped", rep.skipped)
        for c in R.CHECKS + ("H",):
            WORST[(n, c)] = max(WORST.get((n, c), 0.0), rep.worst_of(c))
        asym = B.asymmetry(sg["h_end"])
        assert asym > B.NOT_SYMMETRIC * rep.dh_max, (rep.name, "the matrix is not clearly non-symmetric", asym, rep.dh_max)
    TALLY.add_run(reps)


@pytest.mark.parametrize("kind,n,boxed,lazy,plan", B.REF_CASES, ids=lambda v: B.plan_id(v) if isinstance(v, tuple) else str(v))
def test_three_orders_inside_the_bounds_and_nothing_skipped(kind, n, boxed, lazy, plan):
    for order in Q.ORDERS:
        reps, segs = B.ref_run(kind, n, boxed, lazy, plan[0], plan[1], order)
        _hold(reps, segs, n)


def test_the_blocked_order_agrees_with_the_plain_one():
    """the tile order of BroydenRef is new code: each of its products against numpy's, entry by entry, under ONE bound of a sum of n products
    ((n + 4) eps |m| |v|; the triangle inequality would allow two), on a non-symmetric matrix at every size; and whole runs side by side"""
    for n in B.SIZES:
        rng = np.random.default_rng(n)
        m, v = np.eye(n) + rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal(n)
        bound = (n + 4) * R.EPS
        r_row = R._ratio(B.mvf("blocked", m, v) - m @ v, bound * (np.abs(m) @ np.abs(v)))
        r_col = R._ratio(B.mtv("blocked", m, v) - m.T @ v, bound * (np.abs(m).T @ np.abs(v)))
        r_rev = R._ratio(B.mtv("reversed", m, v) - m.T @ v, bound * (np.abs(m).T @ np.abs(v)))
        print(f"n = {n}: blocked against plain, rows {r_row:.3e}, columns {r_col:.3e}; reversed columns {r_rev:.3e}")
        assert r_row <= 1.0 and r_col <= 1.0 and r_rev <= 1.0
        assert np.max(np.abs(B.mtv("blocked", m, v) - m @ v)) > 1e6 * bound * np.max(np.abs(m) @ np.abs(v))  # (columns, not rows)
    for n in (129, 257):
        worst = {}
        for order in ("plain", "blocked"):
            reps, _ = B.ref_run("synth", n, False, True, (3, 3), True, order)
            worst[order] = max(rep.worst for rep in reps)
        print(f"n = {n}: worst ratio of a run, plain {worst['plain']:.3e}, blocked {worst['blocked']:.3e}")
        assert max(worst.values()) <= 1.0


def test_skip_caps_and_the_record_of_ratios():
    """(behind the replays above: their tally, and the CPU half of the record in tests/broyden_replay_cases.py)"""
    for n in sorted({k[0] for k in WORST}):
        print(f"broyden replay of the float64 runs, n = {n:5d} worst ratios: " + ", ".join(f"{c} {WORST[(n, c)]:.2e}" for c in R.CHECKS + ("H",)))
    print(f"skipped {TALLY.skipped} of {TALLY.triples} (run, iteration, check) triples; the seeded matrix is the {Q.SOURCE.get('synth')}'s")
    assert TALLY.triples > 0 and TALLY.skipped == 0
    TALLY.check()


# ---- planted faults ----
def _rejected(reps):
    return sorted({(i, k, c) for i, rep in enumerate(reps) for k, c, r, a in rep.rows if a and not r <= 1.0})


_clean = {}


def _plant(tag, fault, n, kind="synth", boxed=False, lazy=False, order="blocked", plan=(3, 3)):
    key = (kind, n, boxed, lazy, order, plan)
    if key not in _clean:
        _clean[key] = _rejected(B.ref_run(kind, n, boxed, lazy, plan, True, order)[0])
    assert not _clean[key], (tag, "the clean run must pass")
    bad = _rejected(B.ref_run(kind, n, boxed, lazy, plan, True, order, fault=fault)[0])
    print(f"planted fault {tag} on {kind}{n}: rejected (segment, iteration, check) {bad[:8]}")
    assert bad, (tag, "accepted")
    return bad


@pytest.mark.parametrize("n", B.FAULT_SIZES)
@pytest.mark.parametrize("lazy", [False, True])
def test_fault_w_from_rows(n, lazy):
    bad = _plant("w_rows", ("w_rows",), n, lazy=lazy)
    assert not [x for x in bad if x[0] == 0 and x[1] == 0] and (0, 2, "H") in bad  # (invisible on the first update from I)


@pytest.mark.parametrize("n", B.FAULT_SIZES)
def test_fault_textbook_denominator(n):
    bad = _plant("textbook_den", ("textbook_den",), n)
    assert (0, 2, "H") in bad


@pytest.mark.parametrize("n", B.FAULT_SIZES)
def test_fault_a_row_missing_from_the_column_sums(n):
    for i in sorted({min(128, n - 1), n - 1}):
        bad = _plant(f"col_row_dropped {i}", ("col_row_dropped", i), n)
        assert (0, 2, "H") in bad and not [x for x in bad if x[0] == 0 and x[1] <= 1 and x[2] != "H"]


@pytest.mark.parametrize("n", B.FAULT_SIZES)
@pytest.mark.parametrize("k", [0, 1, 2])
def test_fault_the_edge_entry_not_updated(n, k):
    bad = _plant(f"edge_entry {k}", ("edge_entry", k), n)
    # in its own segment, by H or by a later direction only.  (n = 7, k = 0: rejected by the direction of iteration 1; the faulty run then stalls,
    # s.y = 0 cannot be bounded, and the H check of that segment is skipped, not passed)
    assert [x for x in bad if x[0] == 0] and not [x for x in bad if x[0] == 0 and x[1] <= k and x[2] != "H"]
    assert (0, 2, "H") in bad or (n, k) == (7, 0)


@pytest.mark.parametrize("n", B.FAULT_SIZES)
def test_fault_the_pending_update_applied_twice(n):
    bad = _plant("applied_twice 2", ("applied_twice", 2), n)
    assert not [x for x in bad if x[0] == 0] and (1, 0, "dir") in bad  # the matrix the getter returned was right: the next call's first step is not


@pytest.mark.parametrize("n", B.FAULT_SIZES)
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("k", [1, 2])
def test_fault_a_stale_direction(n, lazy, k):
    bad = _plant(f"stale_dir {k}", ("stale_dir", k), n, lazy=lazy)
    assert bad[0] == (0, k, "dir")


@pytest.mark.parametrize("n", B.FAULT_SIZES)
def test_fault_the_lazy_direction_with_s_g(n):
    bad = _plant("lazy_sg", ("lazy_sg",), n, lazy=True)
    assert (0, 2, "dir") in bad and (0, 1, "dir") not in bad  # (w = s on the first update from I)


# (n = 1024 in the lazy form only: a direction by a pass over H at that size is what tests/test_ref_quad_replay.py's fault 1 already plants)
G_ENTRY = [(n, lazy, k) for n in B.FAULT_SIZES for lazy in (False, True) for k in range(6)] + [(1024, True, k) for k in range(6)]


@pytest.mark.parametrize("n,lazy,k", G_ENTRY)
def test_fault_a_gradient_entry_off_by_1e_9(n, lazy, k):
    bad = _plant(f"g_entry (iteration {k})", ("g_entry", k, 1e-9), n, lazy=lazy)
    assert (k // 3, k % 3, "dir") in bad  # ... by the direction check of that very iteration
