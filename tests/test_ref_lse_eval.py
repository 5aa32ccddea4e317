"""CPU: licenses tests/lse_eval_cases.py, the checker tests/test_gpu_lse_eval.py holds the device to.  Three float64 restatements of the log-sum-exp
evaluation (plain, reversed summation, the kernels' fold over workgroups and ranks) must sit inside the derived bounds on every case, masked ones
included; a float64 DFP / BFGS run on the fold model must replay with every ratio <= 1 and within the skip cap; and every planted fault must be
rejected on its named case -- a checker that accepts them would prove nothing.

The run's oracle is the numpy fold model (lse_eval_cases.eval_fold), not oracle/qn_oracle.c: the C oracle does accept -inf entries of c (its global
maximum and exp(-inf) = 0 give the deleted-rows value; test_c_oracle_accepts_masked_rows), but the fold model is the order the kernels are held to."""
import numpy as np
import pytest

import lse_eval_cases as E

INF = float("inf")


def _worlds(cs):
    return sorted(set((1,) + tuple(cs.worlds)))


_truth0 = {}


def truth0(cs):
    if cs.name not in _truth0:
        a, c, x0 = E.problem(cs.name)
        _truth0[cs.name] = E.Truth(a, c, x0)
    return _truth0[cs.name]


def test_case_table_covers_every_family_and_mechanism():
    fams = {c.family for c in E.CASES}
    assert fams == {"normal", "asc", "desc", "rank_offset", "masked"}
    for fam in fams:
        assert any(1 in c.worlds for c in E.CASES if c.family == fam), fam
    for fam in ("rank_offset", "masked", "normal"):  # what concerns ranks: on 2, 3 and 4 ranks
        assert {w for c in E.CASES if c.family == fam for w in c.worlds} >= {2, 3, 4}, fam
    assert {c.param for c in E.CASES if c.family == "normal"} == {1.0, 300.0, 3000.0}
    assert {c.param for c in E.CASES if c.family == "rank_offset"} == {20.0, 800.0}
    assert {(c.m, c.n) for c in E.CASES} >= {(1, 1024), (5, 1024), (20, 1024), (300, 1152), (1030, 1152), (5, 2176), (5, 4224), (5, 16384)}
    # the grid: m = 20 on 3 and 4 ranks leaves ranks without rows; m = 1030 has 256 workgroups, 50 of them without rows; m = 5 has two with rows
    assert E.grid(20, 3)[0] == E.grid(20, 4)[0] == 16 and E.grid(1030, 1) == (1040, 256, 5) and E.grid(5, 1) == (16, 4, 4)
    assert sum(1 for w in range(256) if E.workgroup_rows(1030, 1, 0, w)[0] >= E.workgroup_rows(1030, 1, 0, w)[1]) == 50
    # a masked case masks the first row of workgroup 0, a whole middle workgroup, the last row and (sharded) every row of rank 1
    for cs in E.CASES:
        if cs.family == "masked":
            c = E.problem(cs.name)[1]
            assert c[0] == -INF and c[-1] == -INF and np.isfinite(c).sum() >= 1
            if cs.mask_world > 1:
                mrpr = E.rows_per_rank(cs.m, cs.mask_world)
                assert np.all(c[mrpr:2 * mrpr] == -INF)
            if cs.m >= 20:
                lo, hi = E.workgroup_rows(cs.m, cs.mask_world, 0, (-(-min(cs.m, E.grid(cs.m, cs.mask_world)[0]) // E.grid(cs.m, cs.mask_world)[2])) // 2)
                assert hi > lo and np.all(c[lo:hi] == -INF)


def test_three_restatements_inside_the_bounds_on_every_case():
    worst = {}
    for cs in E.CASES:
        a, c, x0 = E.problem(cs.name)
        tr = truth0(cs)
        forms = [("plain", E.eval_plain(a, c, x0)), ("reversed", E.eval_reversed(a, c, x0))]
        forms += [(f"fold/{w}", E.eval_fold(a, c, x0, world=w)) for w in _worlds(cs)]
        for form, (f, g) in forms:
            rf, rg = E.point_ratios(tr, f, g)
            assert rf <= 1.0 and rg <= 1.0, (cs.name, form, rf, rg)
            key = (cs.label, form.split("/")[0])
            worst[key] = max(worst.get(key, 0.0), rf, rg)
    for (fam, form), r in sorted(worst.items()):
        print(f"lse restatement {fam:18s} {form:9s} worst ratio {r:.3e}")


def test_masked_truth_is_the_truth_of_the_rows_deleted_and_the_old_row_loop_is_rejected():
    for cs in E.CASES:
        if cs.family != "masked":
            continue
        a, c, x0 = E.problem(cs.name)
        keep = c > -INF
        t_all, t_del = truth0(cs), E.Truth(a[keep], c[keep], x0)
        assert t_all.f == t_del.f and np.array_equal(t_all.g, t_del.g)
        # the row loop as it was (exp(m_run - m_new) with both -inf): a workgroup that BEGINS with a masked row poisons f -- the checker rejects it
        f, g = E.eval_fold(a, c, x0, world=1, select=False)
        assert np.isnan(f) and max(E.point_ratios(t_all, f, g)) == INF, cs.name


def test_c_oracle_accepts_masked_rows(qo):
    cs = E.BY_NAME["m20_n1024_masked"]
    a, c, x0 = E.problem(cs.name)
    f, g = qo.LogSumExpOracle(a, c, E.MU)(x0)
    rf, rg = E.point_ratios(truth0(cs), f, g)
    assert rf <= 1.0 and rg <= 1.0, (rf, rg)


_runs = {}


def _run(cs, method):
    """the float64 run of the case on the fold model (its first world), computed once"""
    if (cs.name, method) not in _runs:
        a, c, x0 = E.problem(cs.name)
        w = cs.worlds[0]
        _runs[(cs.name, method)] = E.reference_run(lambda x: E.eval_fold(a, c, x, world=w), x0, method, cs.iters)
    return _runs[(cs.name, method)]


TALLY, WORST = E.Tally(), {}


@pytest.mark.parametrize("cs", E.CASES, ids=repr)
def test_replay_accepts_the_float64_runs(cs):
    a, c, x0 = E.problem(cs.name)
    for method in ("dfp", "bfgs"):
        tr, xs = _run(cs, method)
        rep = E.replay(f"{cs.name}/{method}", a, c, x0, method, tr, xs)
        E.check(rep)
        TALLY.add(rep)
        WORST[cs.label] = max(WORST.get(cs.label, 0.0), rep.worst)


def test_skip_cap_over_the_float64_runs():
    """(behind the replays above: their tally.  At most 10 % of the (case, iteration, check) triples skipped; iteration 0 and one direction check per
    run are asserted as each run is added.)"""
    for fam, r in sorted(WORST.items()):
        print(f"lse replay of the float64 runs, {fam:18s} worst ratio {r:.3e}")
    print(f"skipped {TALLY.skipped} of {TALLY.triples} (case, iteration, check) triples")
    TALLY.check()


# which case catches which planted fault.  (d): with m_r = -inf the term exp(-inf - M) S_r is an exact 0 whatever S_r holds -- no checker can or should
# reject that; the fault planted is the slot of a rank without rows read as it was allocated, (m_r, S_r) = (0, 1) in place of (-inf, 0)
FAULTS = [
    ("a", "m20_n1024_offset20", 1, "drop"),  # (a row of rank 1's block: p_k of a few 1e-9)
    ("b", "m300_n1152_asc5", 1, ("no_rescale_g",)),
    ("c", "m20_n1024_offset20", 2, ("rank_weight_one", 1)),
    ("d", "m20_n1024_normal1", 4, ("stale_empty_rank",)),
    ("f", "m300_n1152_normal3000", 1, ("f_without_max",)),
]


@pytest.mark.parametrize("tag,name,world,fault", FAULTS, ids=[f[0] for f in FAULTS])
def test_planted_evaluation_faults_are_rejected(tag, name, world, fault):
    cs = E.BY_NAME[name]
    a, c, x0 = E.problem(name)
    tr = truth0(cs)
    if fault == "drop":  # the row of smallest weight that is still >= 1e-9
        p = tr.p.astype(np.float64)
        k = int(tr.keep[np.argmin(np.where(p >= 1e-9, p, INF))])
        assert p[np.flatnonzero(tr.keep == k)[0]] >= 1e-9
        fault = ("drop", k)
    ok, bad = E.eval_fold(a, c, x0, world=world), E.eval_fold(a, c, x0, world=world, fault=fault)
    assert max(E.point_ratios(tr, *ok)) <= 1.0
    rf, rg = E.point_ratios(tr, *bad)
    print(f"planted fault ({tag}) on {name}, {world} rank(s): ratio of f {rf:.3e}, of g {rg:.3e}")
    assert (rf > 1.0) if tag == "f" else (max(rf, rg) > 1.0)
    # ... and as the oracle of a run the replay rejects it at iteration 0
    run = E.reference_run(lambda x: E.eval_fold(a, c, x, world=world, fault=fault), x0, "dfp", 1)
    rep = E.replay(f"{name}/fault {tag}", a, c, x0, "dfp", *run)
    assert rep.worst > 1.0, rep.line()


def test_planted_fault_e_one_entry_of_the_gradient_is_seen_by_the_direction_check_alone():
    """(e) m1_n1024_normal1, BFGS: the entry of the gradient that the direction of iteration 0 is formed from off by 1e-10 |g_j| -- no sum of the trace
    moves beyond its bound; the entrywise direction check rejects the run at that iteration, and nothing else does.  (From iteration 1 on the
    half-width carries what y = g+ - g, a difference of nearly equal gradients, does to H: there the check resolves about 1e-8 of an entry.)"""
    cs = E.BY_NAME["m1_n1024_normal1"]
    a, c, x0 = E.problem(cs.name)
    tk = truth0(cs)
    j = int(np.argmax(np.abs(tk.g).astype(np.float64) / tk.scale))
    run = E.reference_run(lambda x: E.eval_fold(a, c, x), x0, "bfgs", cs.iters, perturb=(0, j, 1e-10))
    rep = E.replay(f"{cs.name}/fault e", a, c, x0, "bfgs", *run)
    print(rep.line())
    bad = {(kk, ch) for kk, ch, r, asserted in rep.rows if asserted and not r <= 1.0}
    assert bad == {(0, "dir")}, bad
