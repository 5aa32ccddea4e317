"""CPU licence of the replay (tests/lbfgs_replay.py) that tests/test_gpu_lbfgs_replay.py applies to the GPU: tests/ref_lbfgs.py's float64 COMPACT
form stands in for the device on every case of lbfgs_cases.REPLAY_CASES, in the summation orders of tests/test_ref_lbfgs.py (numpy.dot, reversed;
its third, reversed on the compact form, is the same run here, so the third order is the even and the odd elements summed apart).  Per case:
every asserted iteration is inside the derived bound (ratio <= 1), at most one fifth of the iterations fail the discrimination condition (none at m = 32, n >= 64), the
ring wraps at least twice where the case exists for that, and each of six seeded faults of the stand-in's direction exceeds the bound by 1e3 at
an asserted iteration of a named case."""
import functools
import math

import numpy as np
import pytest

import lbfgs_cases as C
import lbfgs_replay as LR
import ref_lbfgs as RL
import ref_spg as R
import ref_wolfe as RW
from test_ref_lbfgs import rev_dot


def split_dot(a, b):
    return float(np.dot(a[0::2], b[0::2]) + np.dot(a[1::2], b[1::2]))


DOTS = {"dot": np.dot, "reversed": rev_dot, "split": split_dot}
BY_NAME = {c["name"]: c for c in C.REPLAY_CASES}
FAULTS = {  # fault: the case that must catch it
    "a_oldest_pair_ignored_when_full": "m32-quad-bt-n64",
    "b_gram_entry_from_neighbouring_slot": "m32-quad-bt-n64",
    "c_sy_transposed": "wrap-m5-n2050",
    "d_apply_one_slot_late": "wrap-m3-n7",
    "e_rejected_pair_in_oldest_slot": "concave-m2",
    "f_gamma_from_previous_pair": "wrap-m2-n2050",
}


def faulty_compact(pairs, g, gamma, dot, fault, m):
    """ref_lbfgs.compact with one seeded fault"""
    if fault.startswith("a_") and len(pairs) == m and m > 1:
        pairs = pairs[1:]
    k = len(pairs)
    sy = np.array([[float(dot(si, yj)) for _, yj in pairs] for si, _ in pairs])
    yy = np.array([[float(dot(yi, yj)) for _, yj in pairs] for _, yi in pairs])
    p = np.array([float(dot(s, g)) for s, _ in pairs])
    q = np.array([float(dot(y, g)) for _, y in pairs])
    if fault.startswith("b_") and k >= 3:
        sy[0, k - 1] = sy[1, k - 1]
    r = np.triu(sy.T if fault.startswith("c_") else sy)
    w = np.zeros(k)
    for i in range(k - 1, -1, -1):
        w[i] = (p[i] - float(r[i, i + 1:] @ w[i + 1:])) / r[i, i]
    rhs = (np.diag(sy) * w + gamma * (yy @ w)) - gamma * q
    u = np.zeros(k)
    for i in range(k):
        u[i] = (rhs[i] - float(r[:i, i] @ u[:i])) / r[i, i]
    z = gamma * np.array(g, dtype=np.float64)
    applied = pairs[1:] + pairs[:1] if fault.startswith("d_") else pairs
    for (s, y), ui, wi in zip(applied, u, w):
        z = z + ui * s
        z = z + (gamma * -wi) * y
    return z


class Faulty(RL.LBFGS):
    """the stand-in with a fault in its DIRECTION only: the memory, the commit rule and the loop are the restatement's"""

    def __init__(self, *a, fault, **kw):
        super().__init__(*a, direction="compact", **kw)
        self.fault, self.rejected = fault, None

    def compute_direction(self, eval_x_k):
        g = eval_x_k[1]
        z = g
        if self.pairs:
            pairs = self.pairs
            if self.fault.startswith("e_") and self.rejected is not None and len(pairs) == self.m:
                pairs = [self.rejected] + pairs[1:]
            s, y = pairs[-2] if self.fault.startswith("f_") and len(pairs) >= 2 else pairs[-1]
            with np.errstate(all="ignore"):
                self.gamma = 1.0 if self.unit else float(self.dot(s, y)) / float(self.dot(y, y))
                z = faulty_compact(pairs, g, self.gamma, self.dot, self.fault, self.m)
                gz = float(self.dot(g, z))
            if not (gz > 0.0) or math.isinf(gz):
                self.pairs, self.resets, self.gamma, z = [], self.resets + 1, 1.0, g
        else:
            self.gamma = 1.0
        return R.box_projection(self.x - z, self.lb, self.ub) - self.x

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):
        x, g = self.x, eval_x_k[1]
        step = super().update_next_iterate(line_search, eval_x_k, oracle, direction, max_iter_line_search)
        self.rejected = None if self.updated[-1] else (self.x - x, oracle.fn.grad(self.x) - g)
        return step


def _search(kind, lb, ub, dot):
    if kind == "sw":
        return RW.StrongWolfe(dot=dot)
    return C.line_search(kind, lb, ub, dot)


def standin_run(case, dot=np.dot, fault=None):
    """the float64 stand-in on one case, as a lbfgs_replay.Run"""
    fn, x0, lb, ub = C.replay_problem(case, case["cpu_n"])
    rec = LR.Recorder(fn)
    o = R.CountingOracle(rec)
    if fault:
        s = Faulty(case["tol"], x0, lb, ub, m=case["m"], unit_scaling=case["unit"], dot=dot, fault=fault)
    else:
        s = RL.LBFGS(case["tol"], x0, lb, ub, m=case["m"], unit_scaling=case["unit"], dot=dot, direction="compact")
    run = LR.Run(case["m"], case["unit"], lb, ub, x0, rec)
    ls = _search(case["ls"], lb, ub, dot)
    for _ in range(case["calls"]):
        states = []
        try:
            s.minimize(ls, o, case["iters"], 50, callback=lambda r: states.append((r.stored_pairs(), r.gamma, r.resets)))
        except R.MaxIterReached:
            pass
        run.extend(s.trace_x, [r["t"] for r in s.trace], s.updated[len(run.updated):], states)
    return run


@functools.lru_cache(maxsize=None)
def _report(name, order):
    return LR.replay(standin_run(BY_NAME[name], DOTS[order]))


def check_conditions(case, rep):
    """what a case has to meet whatever ran it: the cap on iterations that prove nothing, and the ring going round twice"""
    cap = 0 if case["m"] == 32 and case["n"] >= 64 else rep.iterations // 5
    assert rep.skipped <= cap, (case["name"], rep.skipped, rep.iterations)
    if case["wraps"]:
        assert rep.commits >= (66 if case["m"] == 32 else 2 * (case["m"] + 1)), (case["name"], rep.commits)
        assert rep.head_advances >= case["m"] + 1
        if case["m"] == 32:
            assert rep.max_k == 32


@pytest.mark.parametrize("order", list(DOTS))
@pytest.mark.parametrize("name", list(BY_NAME))
def test_stand_in_is_inside_the_bound(name, order):
    case = BY_NAME[name]
    rep = _report(name, order)
    LR.check(rep, f"{name} [{order}]")
    check_conditions(case, rep)
    assert rep.iterations == case["iters"] * case["calls"], (rep.iterations, "the run ended early: the case list says how many iterations it replays")


def test_cases_reach_what_they_exist_for():
    reps = {name: _report(name, "dot") for name in BY_NAME}
    assert all(reps[f"reject-m{m}"].commits < reps[f"reject-m{m}"].iterations for m in C.REJECT_MEMORIES)  # pairs were rejected ...
    assert reps["concave-m2"].commits == 2 and reps["concave-m2"].max_k == 2                                 # ... with a full memory
    assert reps["zero-gradient-reset"].resets >= 1
    assert reps["grid-wraps-m5"].max_k == 5
    assert reps["warm-restart"].iterations == 40 and reps["warm-restart"].head_advances > 20
    for ls in ("bt", "btb"):
        for n in (7, 2050):
            run = standin_run(BY_NAME[f"box-{ls}-n{n}"])
            x = run.xs[-1]
            active = int(np.sum((x == run.lb) | (x == run.ub)))
            assert 0 < active < n, (ls, n, active)


def test_free_step_contains_the_interval_of_the_four_operations():
    """without a box the replay follows the step as centre and radius (lbfgs_replay.free_step): that must contain the interval the general
    path derives operation by operation, and be no more than a few eps of |x|, |z|, |t z| wider"""
    rng = np.random.default_rng(11)
    n = 4096
    inf = np.full(n, np.inf)
    for scale_z, scale_dz, t in ((1.0, 1e-13, 1.0), (1e-6, 1e-22, 0.25), (1e3, 1e-9, 2.0 ** -20), (1.0, 0.0, 1.0)):
        x = rng.standard_normal(n)
        z = (scale_z * rng.standard_normal(n)).astype(LR.LD)
        dz = scale_dz * rng.random(n)
        lo, hi = LR.step_interval(x.astype(LR.LD), z, dz, LR.LD(t), -inf, inf)
        mid, rad = LR.free_step(x, x.astype(LR.LD), z, np.abs(z).astype(np.float64), dz, LR.LD(t))
        ld = 8 * float(np.finfo(LR.LD).eps) * (np.abs(x) + np.abs(z).astype(np.float64))  # (the interval's ends are rounded in longdouble themselves)
        assert np.all(mid - rad <= lo + ld) and np.all(hi - ld <= mid + rad)
        slack = (mid + rad - hi).astype(np.float64)
        assert np.all(slack <= 8 * LR.EPS * (np.abs(x) + np.abs(z).astype(np.float64) * (1 + t)) + 1e-11 * rad)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_seeded_fault_is_caught(fault):
    name = FAULTS[fault]
    rep = LR.replay(standin_run(BY_NAME[name], fault=fault))
    print(rep.line(f"{name} with fault {fault}"))
    assert rep.worst >= 1e3, (fault, name, rep.worst)
