"""CPU tests of tests/newton_cg_audit.py on the float64 restatement's own whole runs (ref_newton_cg.NewtonCG, ref_newton_pcg.JacobiNewtonCG): every
check passes on every kind, plain and Jacobi, in three summation orders and in the moved runs; the conditions of the licence hold; MARGIN is
measured; and nine planted faults, each in a restatement subclass, are rejected on a licensed direction beyond iteration 6 by at least 100 times the
bound of the check that caught them.  No GPU."""
import math

import numpy as np
import pytest

import newton_cg_audit as AU
import newton_cg_cases as NC
import ref_logistic as RL
import ref_newton_cg as RN
import ref_newton_pcg as RP

ORDERS = [("numpy", None), ("fsum", None), ("reversed", None), ("numpy", 1), ("numpy", 2)]
# the badly scaled runs have 1300 to 2960 inner steps: math.fsum of every product row by row is left to the unscaled cases
PRECOND_ORDERS = [("numpy", None), ("reversed", None), ("numpy", 1)]
_reports = {}


def report(case, order="numpy", seed=None):
    key = (case, order, seed)
    if key not in _reports:
        run, _, status = AU.ref_run(case, order, seed)
        _reports[key] = (AU.audit(run), status)
    return _reports[key]


def _licensed_where_due(rep, up_to=None):
    """(directions with inner steps and positive curvature throughout, how many of them are licensed); up_to: only those with j_k <= up_to"""
    due = [r for r in rep["rows"] if r["j"] >= 1 and r["ended"] in ("tol", "cap") and (up_to is None or r["j"] <= up_to)]
    return len(due), sum(1 for r in due if r["licensed"])


# ---- 1. the restatement's runs pass, and the conditions hold ----
@pytest.mark.parametrize("case", AU.LSE_CASES + AU.UNSCALED_CASES, ids=str)
def test_unscaled_runs_pass_and_every_direction_is_licensed(case):
    for order, seed in ORDERS:
        rep, status = report(case, order, seed)
        print(AU.line(rep), status)
        assert rep["directions"] >= 5 and not rep["failures"], rep["failures"]
        due, licensed = _licensed_where_due(rep)
        assert due == rep["directions"] and licensed == due and rep["ties"] == 0, (due, licensed, rep["ties"])


@pytest.mark.parametrize("case", AU.PRECOND_CASES, ids=str)
def test_badly_scaled_runs_pass_and_short_loops_are_licensed(case):
    """(a) and (b) hold every direction of runs with up to 43 outer iterations and 2964 inner steps; (c) and (d) the licensed ones, among them every
    direction of at most 8 inner steps"""
    for order, seed in PRECOND_ORDERS:
        rep, status = report(case, order, seed)
        print(AU.line(rep), status)
        assert status == "ok" and not rep["failures"], rep["failures"]
        assert rep["worst"]["b"] > 0.0  # (the contract was asserted at all)
        due, licensed = _licensed_where_due(rep, up_to=8)
        assert due >= 3 and licensed == due, (due, licensed)
    rep = report(case)[0]
    inner = sum(r["j"] for r in rep["rows"])
    print(f"{case}: {rep['directions']} outer, {inner} inner; licensed share {rep['licensed']} / {rep['directions']}; (b) without slack {rep['inside_b']:.4f}")
    assert rep["inside_b"] <= 1.0  # (the issue's observation, 0.9961 at the most: the slack is not what makes (b) pass on the restatement)


def test_cap_exits_and_negative_curvature_are_audited():
    """max_inner = 2: cap exits are held by (a) and (c) and never by (b), (d); the negative-mu case: rule 4 at j = 0 leaves d = -g bit for bit"""
    run, s, _ = AU.ref_run(("lse", 96, 64, "bt"), max_inner=2)
    rep = AU.audit(run)
    print(AU.line(rep))
    assert "cap" in s.why and not rep["failures"]
    assert all(r["b"] is None and r["d_late"] is None for r in rep["rows"] if r["ended"] == "cap") and rep["licensed"] == rep["directions"]
    a, c, _, _ = NC.problem(3, 5)
    s = NC.run_ref(3, 5, "bt", iters=0, mu=NC.NEG_MU)[0]
    AU.adopt(s)
    NC.run_ref(3, 5, "bt", iters=3, mu=NC.NEG_MU, solver=s)
    rep = AU.audit(AU.run_of(s, AU.LseOps(a, c, NC.NEG_MU), "lse (3, 5) negative mu"))
    print(AU.line(rep))
    assert rep["rows"][0]["ended"] == "negcurv" and rep["rows"][0]["j"] == 0 and not rep["failures"]
    run = AU.run_of(s, AU.LseOps(a, c, NC.NEG_MU))
    run.dirs[0].d = run.dirs[0].d * (1.0 + 2.0 ** -52)  # a direction that is not -g bit for bit
    assert (0, "a", AU.INF) in AU.audit(run)["failures"]


def test_margin_is_measured():
    """one order stand-in held out at a time over every direction of every CPU case above"""
    orders, moved = 0.0, 0.0
    for case in AU.LSE_CASES + AU.UNSCALED_CASES:
        for order, seed in ORDERS:
            o, m = AU.held_out_ratio(report(case, order, seed)[0])
            orders, moved = max(orders, o), max(moved, m)
    for case in AU.PRECOND_CASES:
        for order, seed in PRECOND_ORDERS:
            o, m = AU.held_out_ratio(report(case, order, seed)[0])
            orders, moved = max(orders, o), max(moved, m)
    margin = max(4.0, float(math.ceil(2.0 * orders)))
    print(f"MARGIN: largest held-out ratio of an order stand-in {orders:.3f} -> MARGIN {margin:g} (newton_cg_audit.MARGIN = {AU.MARGIN:g}); "
          f"the moved stand-in held out, for the record: {moved:.3g}")
    assert margin == AU.MARGIN


# ---- 2. planted faults, each in a restatement subclass ----
class _Faulty:
    """rules 1 to 8 (2', 5', 7' with a diagonal) with one fault planted; fault = None is the restatement operation for operation (asserted below)"""
    fault, fault_from = None, 0

    def compute_direction(self, eval_x_k):
        g, dot = eval_x_k[1], self.dot
        jacobi = hasattr(self, "diag_at")
        k = len(self.inner)
        on = self.fault if k >= self.fault_from else None
        x_prev, self._x_last = getattr(self, "_x_last", self.x), self.x.copy()
        hv = self.hess_vec_at(x_prev if on == "stale_weights" else self.x)
        if on in ("no_gbar", "row_dropped"):
            hv = self.faulty_product(self.x)
        minv = RP.minv_of(self.diag_at(self.x))[0] if jacobi else None
        if jacobi:
            self.diag_passes += 1
            self.floored.append(0)
        z, r = np.zeros_like(g), g.copy()
        p = minv * g if jacobi and on != "no_minv_in_first_p" else g.copy()
        gg = float(dot(g, g))
        rho = float(dot(r, minv * r)) if jacobi else gg
        rho_before = rho
        sqgg = math.sqrt(gg)
        s4 = math.sqrt(sqgg)
        eta = s4 if s4 < self.eta_max else self.eta_max
        if on == "eta_linear":
            eta = sqgg if sqgg < self.eta_max else self.eta_max
        j, zg, gz, alpha_before = 0, False, 0.0, None
        while True:
            q = hv(p)
            self.hv_passes += 1
            kappa = float(dot(p, q))
            if not (kappa > 0.0) or math.isinf(kappa):
                self.neg_curv += 1
                zg = j == 0
                why = "negcurv"
                break
            alpha = RN._div(rho, kappa)
            z = z + alpha * p
            r = r - (alpha_before if on == "alpha_of_the_step_before_in_r" and alpha_before is not None else alpha) * q
            alpha_before = alpha
            j += 1
            y = minv * r if jacobi else r
            rrn, gz = float(dot(r, r)), float(dot(g, z))
            rhon = float(dot(r, y)) if jacobi else rrn
            tested = rhon if on == "test_on_rz" else rrn
            if math.sqrt(tested) <= eta * sqgg:
                why = "tol"
                break
            if j >= self.cap:
                why = "cap"
                break
            beta = RN._div(rho, rho_before) if on == "beta_of_the_step_before" else RN._div(rhon, rho)
            rho_before, rho = rho, rhon
            p = y + beta * p
        if zg:
            d = -g
        elif not (gz > 0.0) or math.isinf(gz) or (on == "fallback_keeps_z" and k == self.fault_from):
            self.fallbacks += 1
            why += "+fallback"
            d = -z if on == "fallback_keeps_z" else -g
        else:
            d = -z
        self.inner.append(j)
        self.why.append(why)
        self.directions.append(d)
        return d


class FaultyNewtonCG(_Faulty, RN.NewtonCG):
    pass


class FaultyJacobiNewtonCG(_Faulty, RP.JacobiNewtonCG):
    pass


LSE, LOGISTIC, JACOBI = ("lse", 257, 200, "bt"), ("logistic", 96, 64, "bt"), ("precond", "dense", 96, 64, "bt", "jacobi")


def _lse_without_gbar(s):
    a, c, mu, _ = NC.problem(LSE[1], LSE[2])
    at = np.ascontiguousarray(a.T)

    def at_x(x):
        z = a @ x + c
        e = np.exp(z - z.max())
        p = e / e.sum()
        return lambda v: at @ (p * (a @ v)) + mu * v
    s.faulty_product = at_x


def _logistic_without_a_row(s):
    import logistic_cases as LC
    a, y, w, mu, _, _ = LC.problem(LOGISTIC[1], LOGISTIC[2])
    at = np.ascontiguousarray(a.T)
    row = int(np.argmax(w))  # a row that carries weight

    def at_x(x):
        d = RL.weights_f64(a, y, w, x).copy()
        d[row] = 0.0
        return lambda v: at @ (d * (a @ v)) + mu * v
    s.faulty_product = at_x


BIG_DIAGONAL = ("big diagonal", "dense", 96, 64, "bt", 1e4)


def _big_diagonal_run(prep=None, weights=BIG_DIAGONAL[5], tol=1e-5):
    """precond_cases' dense (96, 64) problem with its weights and mu multiplied by `weights` (the same minimiser, H and its diagonal that much
    larger), JacobiNewtonCG + BackTracking to ||g||_inf < tol: (Run, solver, status)"""
    import precond_cases as PC
    import ref_spg as R
    pr = PC.problem(BIG_DIAGONAL[2], BIG_DIAGONAL[3], BIG_DIAGONAL[1])
    a, y, w, mu = pr["a"], pr["y"], pr["w"] * weights, pr["mu"] * weights
    s = FaultyJacobiNewtonCG(tol, pr["x0"], RL.logistic_hess_vec_at(a, y, w, mu), RP.logistic_diag_at(a, y, w, mu))
    if prep is not None:
        prep(s)
    AU.adopt(s)
    status = "ok"
    try:
        s.minimize(R.BackTracking(1e-4, 0.5), R.CountingOracle(RL.logistic_fn(a, y, w, mu)), PC.ITERS, PC.MAX_LS)
    except R.MaxIterReached:
        status = "max_iter"
    return AU.run_of(s, AU.LogisticOps(a, y, w, mu), str(BIG_DIAGONAL)), s, status


FAULT_FROM = 7  # planted from the eighth direction on: the windows of today's tests (often the first 6 iterations) see none of them
LAST = -1       # planted at the last direction of the run without the fault
SPARSE_JACOBI = ("precond", "sparse", 96, 64, "bt", "jacobi")
# (fault, case, what prepares the subclass, the first direction that carries it)
FAULTS = [
    ("stale_weights", LOGISTIC, None, FAULT_FROM),
    ("no_gbar", LSE, _lse_without_gbar, FAULT_FROM),
    ("row_dropped", LOGISTIC, _logistic_without_a_row, FAULT_FROM),
    ("beta_of_the_step_before", LOGISTIC, None, FAULT_FROM),
    ("alpha_of_the_step_before_in_r", LOGISTIC, None, FAULT_FROM),
    ("eta_linear", LSE, None, FAULT_FROM),
    # the violation of rule 6 on rz is ||r|| / (eta ||g||) <= min(sqrt(rr / rz), 1 / eta): on precond_cases' own problems sqrt(rr / rz) is 2.4 to 6.3
    # on every Jacobi case (the faulty loop is still rejected there, by (b) and (d), but not a hundredfold).  With the weights 1e4 times larger the
    # diagonal is, the faulty loop ends at j = 1, and at the run's last direction eta is small enough: 230 times the bound
    ("test_on_rz", BIG_DIAGONAL, None, LAST),
    ("no_minv_in_first_p", SPARSE_JACOBI, None, FAULT_FROM),
    ("fallback_keeps_z", LOGISTIC, None, FAULT_FROM),
]
REJECTION = 100.0


def _run_with(fault, case, prepare, fault_from=FAULT_FROM):
    def prep(s):
        s.fault, s.fault_from = fault, fault_from
        if prepare is not None:
            prepare(s)
    if case == BIG_DIAGONAL:
        return _big_diagonal_run(prep)
    cls = FaultyJacobiNewtonCG if case[0] == "precond" and case[-1] == "jacobi" else FaultyNewtonCG
    return AU.ref_run(case, solver_class=cls, prepare=prep)


@pytest.mark.parametrize("case", [LSE, LOGISTIC, JACOBI], ids=str)
def test_the_subclass_without_a_fault_is_the_restatement(case):
    run, s, _ = _run_with(None, case, None)
    ref, r, _ = AU.ref_run(case)
    assert s.inner == r.inner and s.why == r.why and len(run.dirs) == len(ref.dirs) >= FAULT_FROM + 3
    assert all(p.d.tobytes() == q.d.tobytes() and p.x_next.tobytes() == q.x_next.tobytes() for p, q in zip(run.dirs, ref.dirs))


_table = []


@pytest.mark.parametrize("fault,case,prepare,first", FAULTS, ids=[f[0] for f in FAULTS])
def test_planted_fault_is_rejected(fault, case, prepare, first):
    if first == LAST:
        clean = _run_with(None, case, None)[0]
        assert not AU.audit(clean)["failures"]
        first = len(clean.dirs) - 1
    assert first >= FAULT_FROM
    run, s, status = _run_with(fault, case, prepare, first)
    rep = AU.audit(run)
    assert not [f for f in rep["failures"] if f[0] < first], rep["failures"]  # (nothing is wrong before the fault is)
    caught = [(k, c, ratio) for (k, c, ratio) in rep["failures"] if k >= first and rep["rows"][k]["licensed"]]
    best = max(caught, key=lambda f: f[2], default=None)
    seen_by = sorted({c for _, c, _ in caught})
    _table.append((fault, case, first, best, seen_by))
    print(f"fault {fault} on {case} from direction {first}: {len(run.dirs)} directions ({status}); rejected by {seen_by}; strongest: {best}")
    print("fault table so far (fault, case, first faulty direction, (direction, check, ratio to its bound), every check that rejected it):")
    for row in _table:
        print("   ", row)
    assert best is not None and best[2] >= REJECTION, (fault, rep["failures"])
    if fault == "eta_linear":
        assert seen_by == ["d_early"], seen_by  # (a smaller eta only makes the loop run on: the contract (b) and the iterate (c) cannot see it)
