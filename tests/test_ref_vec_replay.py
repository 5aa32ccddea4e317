"""CPU licence of the step-by-step replay (tests/vec_replay.py) on the float64 restatements tests/ref_spg.py and tests/ref_pnewton.py:

  * every case of tests/vec_replay_cases.py in three summation orders (numpy.dot, math.fsum, reversed): every ratio at most 1, every equality
    exact, NO skipped iteration and NO undecidable decision (a case that fails this is replaced, the cap is never loosened), and the
    conditions each case was chosen for;
  * call plans (6,), (3, 3), (1, 2, 3) give one x-trace byte for byte;
  * fifteen planted faults (the issue's fourteen, and a ring one value short), each a small variant of the restatement: the same checker rejects
    each on at least one listed case, and through a quantity the fault touches.

Run with -s for the worst ratio per quantity."""
import math

import numpy as np
import pytest

import lbfgs_replay as LR
import ref_pnewton as RP
import ref_spg as R
import vec_replay as VR
import vec_replay_cases as C

LD = np.longdouble


def rev_dot(a, b):
    return float(np.dot(a[::-1].copy(), b[::-1].copy()))


ORDERS = {"numpy": np.dot, "fsum": R.fsum_dot, "reversed": rev_dot}


class MemoOracle:
    """the closure behind a memo of the last point evaluated: `calls` counts the reference's sequence, `evals` the evaluations made"""

    def __init__(self, rec, memoize, newton):
        self.rec, self.memoize, self.newton = rec, memoize, newton
        self.calls = self.evals = 0
        self.held = self.last = None
        self.in_search = False  # a trial is always evaluated: the memo serves the loop top and the evaluation at x_next alone

    def start_call(self):
        self.calls = self.evals = 0
        self.held = None

    def __call__(self, x):
        self.calls += 1
        k = VR.key(x)
        if not (self.memoize and not self.in_search and self.held == k):
            self.evals += 1
            res = self.rec(np.array(x, dtype=np.float64))
            self.last = res if self.newton else (res[0], np.asarray(res[1]))  # (HRecorder hands out ref_pnewton.Eval)
            self.held = k
        return self.last


class GLL(R.GLLQuadratic):
    """ref_spg.GLLQuadratic with the planted faults 3, 5, 6, 15 behind switches"""
    fault = None

    def append_new_f(self, f):
        if len(self.f_previous) == self.m + {3: 1, 15: -1}.get(self.fault, 0):
            self.f_previous.pop(0)
        self.f_previous.append(f)

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):
        if self.fault not in (5, 6):
            return super().compute_step_len(x_k, eval_x_k, direction_k, oracle, max_iter)
        f_k, g_k = eval_x_k
        self.append_new_f(f_k)
        t, f_max, i, self.trials = 1.0, self.f_max(), 0, 0
        gd = float(self.dot(g_k, direction_k))
        while max_iter > i:
            f_kp1, _ = oracle(x_k + t * direction_k)
            self.trials += 1
            if f_kp1 - f_max <= self.c1 * t * gd:
                return t
            if t <= 0.1:
                t *= 0.5
            else:
                t_tmp = -0.5 * t * t * gd / (f_kp1 - (f_max if self.fault == 5 else f_k) - t * gd)
                if t_tmp > self.sigma1 and t_tmp < (self.sigma2 if self.fault == 6 else self.sigma2 * t):
                    t = t_tmp
                else:
                    t = t_tmp * 0.5
            i += 1
        return t


class BTB(R.BackTrackingB):
    fault = None

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):
        if self.fault != 10:
            return super().compute_step_len(x_k, eval_x_k, direction_k, oracle, max_iter)
        f_k, _ = eval_x_k
        t, i, self.trials = 1.0, 0, 0
        while max_iter > i:
            f_kp1, _ = oracle(R.box_projection(x_k + t * direction_k, self.lb, self.ub))
            self.trials += 1
            diff = t * direction_k  # fault 10: the unprojected trial
            if f_kp1 - f_k <= (-self.c1 / t) * float(self.dot(diff, diff)):
                return t
            t *= self.beta
            i += 1
        return t


def _faulty(base, fault):
    class Faulty(base):
        def projected_gradient(self, eval_x_k):
            if fault == 2:
                return np.array(eval_x_k[1], dtype=np.float64)
            return super().projected_gradient(eval_x_k)

        def compute_direction(self, eval_x_k):
            if fault == 1 and hasattr(self, "lam") and base is R.SpectralProjectedGradient:
                u = (self.x.astype(LD) - LD(self.lam) * eval_x_k[1].astype(LD)).astype(np.float64)
                d = R.box_projection(u, self.lb, self.ub) - self.x
            else:
                d = super().compute_direction(eval_x_k)
            self.last_d = d
            return d

        def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):
            if fault in (7, 8, 9, 13) and base is R.SpectralProjectedGradient:
                step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
                nxt = self.x + step * direction
                s = nxt - self.x
                gn = oracle.last[1] if fault == 13 else oracle(nxt)[1]
                if fault == 13:
                    oracle.calls += 1
                y = gn - eval_x_k[1]
                self.x = nxt
                ss = float(self.dot(s[:4096], s[:4096])) if fault == 9 else float(self.dot(s, s))
                self.last_s_norm = math.sqrt(ss)
                sy = float(self.dot(s, y))
                if sy <= 0.0:
                    self.lam = self.lambda_min if fault == 8 else self.lambda_max
                    return step
                self.lam = R.rmax(R.rmin(sy / ss if fault == 7 else ss / sy, self.lambda_max), self.lambda_min)
                return step
            if fault in (11, 12) and base is R.ProjectedGradientDescent:
                step = line_search.compute_step_len(self.x, eval_x_k, direction, oracle, max_iter_line_search)
                self.x = self.x + step * direction
                if fault == 12:
                    self.x = R.box_projection(self.x, line_search.lb, line_search.ub)
                else:
                    oracle.held = VR.key(self.x)  # "moved" ignored: the projected trial's evaluation passes for x_next's
                return step
            step = super().update_next_iterate(line_search, eval_x_k, oracle, direction, max_iter_line_search)
            if fault == 14 and base is RP.ProjectedNewton:
                self.s_norm = self.last_s_norm = math.sqrt(float(self.dot(direction, direction)))
            return step
    return Faulty


def _seq_dot(a, b):
    acc = 0.0
    for u, v in zip(a.tolist(), b.tolist()):
        acc = acc + u * v
    return acc


def _small_dot(dot, n):
    """the substitution's sums: in index order up to n = 5, where pn_small_kernel is nalgebra operation for operation"""
    return _seq_dot if n <= VR.SMALL_N else dot


def ref_run(case, dot=np.dot, fault=None):
    """the restatement on one case, recorded as the GPU test records the device -> vec_replay.Run"""
    fn, x0, lb, ub = C.problem(case)
    method, newton = case["method"], case["method"] in ("pn", "spn")
    rec = VR.HRecorder(fn, lambda f, g, h, _read: RP.Eval(f, g, h)) if newton else LR.Recorder(lambda x: fn(x)[:2], keep_x=True)
    o = MemoOracle(rec, case["memoize"], newton)
    spec = C.line_search(case, lb, ub, fn)
    if spec["kind"] == "gll":
        ls = GLL(spec["c1"], spec["m"], dot=dot).with_sigmas(spec["sigma1"], spec["sigma2"])
    elif spec["kind"] == "bt":
        ls = R.BackTracking(spec["c1"], spec["beta"], dot=dot)
    else:
        ls = BTB(spec["c1"], spec["beta"], spec["lo"], spec["hi"], dot=dot)
    ls.fault = fault
    inner = ls.compute_step_len

    def compute_step_len(*a):
        o.in_search = True
        try:
            return inner(*a)
        finally:
            o.in_search = False
    ls.compute_step_len = compute_step_len
    lmin, lmax = case.get("lambdas", (1e-3, 1e3))
    run = VR.Run(method, spec, lb, ub, x0, rec, case["memoize"], case["max_ls"], case["tol"], lmin, lmax, limited=case.get("limited", False))
    tol = case["tol"]
    if method == "spg":
        s = _faulty(R.SpectralProjectedGradient, fault)(tol, x0, o, lb, ub, dot=dot)
    elif method == "pgd":
        s = _faulty(R.ProjectedGradientDescent, fault)(tol, x0, lb, ub)
    elif method == "pn":
        s = _faulty(RP.ProjectedNewton, fault)(tol, x0, lb, ub, solve=RP.CholeskySolve(_small_dot(dot, x0.size)), dot=dot)
    else:
        s = _faulty(RP.SpectralProjectedNewton, fault)(tol, x0, o, lb, ub, solve=RP.CholeskySolve(_small_dot(dot, x0.size)), dot=dot)
    if method in ("spg", "spn"):
        s.with_lambdas(lmin, lmax)
        run.lam0 = s.lam
    run.grads.append(rec.seen[VR.key(run.x0)][1] if VR.key(run.x0) in rec.seen else None)
    for iters in case["plan"]:
        o.start_call()
        if fault == 4 and spec["kind"] == "gll":
            ls.f_previous = []
        seen = []

        def cb(sv):
            seen.append(dict(d=sv.last_d.copy(), lam=getattr(sv, "lam", None), s_norm=getattr(sv, "last_s_norm", None), y_norm=getattr(sv, "last_y_norm", None)))
        converged = True
        try:
            s.minimize(ls, o, iters, case["max_ls"], callback=cb)
        except R.MaxIterReached:
            converged = False
        tr = [dict(r, y_norm=sn["y_norm"] if method == "pn" else 0.0) for r, sn in zip(s.trace, seen)]
        run.add_call(tr, s.trace_x, seen, o.calls, o.evals, converged)
        if run.limited:
            run.grads += [rec.seen[VR.key(x)][1] for x in s.trace_x]
    return run


def _x_trace(run):
    return b"".join(it["x"].tobytes() for c in run.calls for it in c["its"])


TALLY = {}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_restatement_inside_the_bounds(case, order):
    rep = VR.replay(ref_run(case, dot=ORDERS[order]))
    VR.check(rep, f"{case['name']} [{order}]")
    C.check_conditions(case, rep)
    for q, v in rep.worst.items():
        TALLY[q] = max(TALLY.get(q, 0.0), v)
    TALLY["first decision: bound / margin"] = max(TALLY.get("first decision: bound / margin", 0.0), rep.first_margin)


def test_tally():
    print("\nworst ratio per quantity over the cases run in this session:")
    for q, v in TALLY.items():
        print(f"  {q:32s} {v:.3e}")


def test_every_gll_branch_is_met():
    seen = {b: 0 for b in C.BRANCHES}
    for case in C.CASES:
        if case["ls"] == "gll" and case["n"] <= 4099:
            rep = VR.replay(ref_run(case))
            for b in C.BRANCHES:
                seen[b] += rep.branches[b]
    assert all(v >= 1 for v in seen.values()), seen


def test_call_plans_give_one_trace():
    group = [c for c in C.CASES if c.get("group") == "plan"]
    assert [c["plan"] for c in group] == [(6,), (3, 3), (1, 2, 3)]
    traces = [_x_trace(ref_run(c)) for c in group]
    assert traces[0] == traces[1] == traces[2]


def _by_name(name):
    return next(c for c in C.CASES if c["name"] == name)


# fault: (what, the quantities of the checker that the fault touches -- a rejection counts only when one of them trips --, the cases)
FAULTS = {
    1: ("x - lam g rounded once", {"d"}, ["spg-gll-spd-2049", "spg-gll-spd-17"]),
    2: ("a bound-sitting entry not zeroed in gnorm", {"gnorm"}, ["spg-gll-crafted-16", "pgd-btb-crafted-2048"]),
    3: ("f_max over m + 1 values", {"trial", "t", "counts"}, ["spg-gll-chain-17-m1", "spg-gll-ring-7", "spg-gll-chain-16-m10"]),
    4: ("the ring cleared between calls", {"trial", "t", "counts"}, ["spg-gll-plan-3-3", "spg-gll-plan-1-2-3"]),
    5: ("t_tmp with f_max in place of f_k", {"trial", "t"}, ["spg-gll-chain-2049", "spg-gll-spd4-4099-lambdas", "spg-gll-chain-2047-steep", "spg-gll-chain-16-narrow"]),
    6: ("sigma2 compared instead of sigma2 t", {"trial", "t"}, ["spg-gll-chain-17-strict", "spg-gll-chain-2048-strict"]),
    7: ("lambda = sy / ss", {"lambda"}, ["spg-gll-spd-2049", "spg-gll-spd-7"]),
    8: ("sy <= 0 -> lambda_min", {"lambda"}, ["spg-gll-chain-2049"]),
    9: ("the last workgroup's share of s.s dropped at G = 3", {"s_norm", "lambda"}, ["spg-gll-spd-4099", "spg-gll-crafted-4099"]),
    10: ("BackTrackingB's diff2 from the unprojected trial", {"trial", "t", "counts"}, ["pgd-btb-crossing-17", "pgd-btb-crossing-2049"]),
    11: ("'moved' ignored: one evaluation fewer", {"sequence", "counts"}, ["pgd-btb-crafted-17", "pgd-btb-crafted-2047", "pgd-btb-crafted-2049"]),
    12: ("x_next set to the projected trial", {"x_next"}, ["pgd-btb-crafted-16", "pgd-btb-crafted-2048"]),
    13: ("the evaluation at x_next skipped with memoize 0", {"sequence", "counts"}, ["spg-gll-spd-1", "spg-gll-spd-5", "spg-gll-spd-2049"]),
    14: ("ProjectedNewton's s_norm from ||d||", {"s_norm"}, ["pn-gll-quartic-6", "pn-gll-quartic-17", "pn-bt-quartic-5"]),
    15: ("f_max over m - 1 values", {"trial", "t", "counts"}, ["spg-gll-ring-7", "spg-gll-chain-16-m10"]),
}


@pytest.mark.parametrize("fault", list(FAULTS), ids=[f"{k}-{v[0].replace(' ', '_')}" for k, v in FAULTS.items()])
def test_planted_fault_is_rejected(fault):
    what, touched, names = FAULTS[fault]
    rejected = []
    for name in names:
        case = _by_name(name)
        if fault in (11,) and not case["memoize"]:
            continue
        if fault == 13 and case["memoize"]:
            continue
        rep = VR.replay(ref_run(case, fault=fault))
        hits = [p for p in rep.problems if p[1] in touched]
        if hits:
            rejected.append((name, hits[0]))
    print(f"fault {fault} ({what}): rejected on {[(n, p[1], p[3]) for n, p in rejected]}")
    assert rejected, (fault, what, names)
