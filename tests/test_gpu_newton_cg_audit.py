"""GPU: every direction of whole NewtonCG runs audited in extended precision by tests/newton_cg_audit.py -- (a) the bookkeeping bit for bit, (b) the
inexact-Newton contract with its derived slack, (c) the iterate against the extended one where float64 can tell, (d) the stopping step -- on all five
objectives, plain and Jacobi, to convergence: the iterations behind the licensed windows of the other NewtonCG tests, where so far only "it
converged" was checked.  The recorder reads d_k and g_{k+1} in the callback through qn_solver_get_direction / qn_solver_get_gradient
(NewtonCG.direction(), .gradient()): the audit needs the run's own vectors bit for bit.  g_0, and every g_k of a run that is not memoised (which
holds no evaluation at x when the callback runs: the getter refuses), is the objective's public evaluation at x_k -- the launches the solver's own
evaluation makes, and asserted equal bit for bit to every gradient the getter did return.  (An iteration cap of 0 evaluates nothing, as in the
reference: there is no g_0 to read after such a call.)

Each test prints its table: directions, those with inner steps, licensed, ties, the worst ratio of each check.  It is a record, not a tolerance: the
bounds are newton_cg_audit's, derived or measured on the CPU."""
import numpy as np
import pytest

import logistic_cases as LC
import multinomial_cases as MC
import newton_cg_audit as AU
import newton_cg_cases as NC
import precond_cases as PC
import sparse_logistic_cases as SL
import sparse_multinomial_cases as SM

pytestmark = pytest.mark.gpu
_worst = {}


def _objective(qn, case, mu=None):
    """(the device objective, x0) of a case of newton_cg_audit"""
    fam = case[0]
    if fam == "lse":
        a, c, mu0, x0 = NC.problem(case[1], case[2])
        return qn.LogSumExp(a, c, mu0 if mu is None else mu), x0
    if fam == "logistic":
        a, y, w, mu0, x0, _ = LC.problem(case[1], case[2])
        return qn.Logistic(a, y, mu0, weights=w), x0
    if fam == "slogistic":
        pr = SL.problem(case[1], case[2])
        return qn.SparseLogistic(pr["indptr"], pr["indices"], pr["data"], pr["y"], pr["mu"], pr["a"].shape[1], weights=pr["w"]), pr["x0"]
    if fam == "multinomial":
        a, y, w, k, mu0, x0, _ = MC.problem(*case[1:4])
        return qn.Multinomial(a, y, k, mu0, weights=w), x0
    if fam == "smultinomial":
        pr = SM.problem(*case[1:4])
        return qn.SparseMultinomial(pr["indptr"], pr["indices"], pr["data"], pr["y"], pr["k"], pr["mu"], pr["a"].shape[1], weights=pr["w"]), pr["x0"]
    pr = PC.problem(case[2], case[3], case[1])
    if case[1] == "sparse":
        return qn.SparseLogistic(pr["indptr"], pr["indices"], pr["data"], pr["y"], pr["mu"], pr["a"].shape[1], weights=pr["w"]), pr["x0"]
    return qn.Logistic(pr["a"], pr["y"], pr["mu"], weights=pr["w"]), pr["x0"]


def record(qn, case, ops=None, iters=None, calls=1, memoize=1, chunk=8, max_inner=0, mu=None):
    """one NewtonCG run of a case through `minimize` (`calls` successive calls of `iters` iterations, audited as one): (newton_cg_audit.Run, status,
    stats of the last call)"""
    precond = case[-1] if case[0] == "precond" else "none"
    ls_kind = case[-2] if case[0] == "precond" else case[-1]
    iters = iters or (PC.ITERS if case[0] == "precond" else NC.ITERS)
    obj, x0 = _objective(qn, case, mu)
    s = qn.NewtonCG(NC.TOL, x0, max_inner=max_inner, chunk=chunk, memoize=memoize, preconditioner=precond)
    run = AU.Run(ops or AU.ops_of(case), max_inner if max_inner > 0 else min(x0.size, 100), 0.5, precond == "jacobi",
                 f"{case} memoize={memoize} chunk={chunk}" + (f" max_inner={max_inner}" if max_inner else "") + (f" calls={calls}" if calls > 1 else ""))
    status, got = "ok", []  # got: the gradients the getter returned, with their points
    try:
        x, g = np.array(x0, dtype=np.float64), obj(x0).g()
        neg_base = fb_base = 0
        for _ in range(calls):
            s.set_trace(iters, with_x=True)
            rec = []

            def callback(sv):
                minv = sv.preconditioner_diag()[1] if precond == "jacobi" else None
                rec.append((sv.x(), sv.direction(), sv.gradient() if memoize else None, sv.inner_iterations()[0], sv.negative_curvature(), sv.fallbacks(), minv))
            try:
                s.minimize(qn.StrongWolfe(*NC.WOLFE) if ls_kind == "wolfe" else qn.BackTracking(1e-4, 0.5), obj, iters, NC.MAX_LS, callback=callback)
            except qn.MaxIterReached:
                status = "max_iter"
            tr, xs = s.trace()
            assert len(tr) == len(rec)
            neg = fb = 0
            for r, (x_next, d, g_next, j, neg1, fb1, minv) in zip(tr, rec):
                run.dirs.append(AU.Direction(x, g, d, r["t"], x_next, j, neg_base + neg, neg_base + neg1, fb_base + fb, fb_base + fb1, minv))
                if g_next is not None:
                    got.append((x_next, g_next))
                neg, fb, x = neg1, fb1, x_next
                g = g_next if g_next is not None else np.zeros_like(x)  # (a run that is not memoised: filled in below)
            assert all(np.array(a).tobytes() == b[0].tobytes() for a, b in zip(xs, rec))  # (the trace's iterates are the callback's)
            neg_base, fb_base = neg_base + neg, fb_base + fb
        stats = s.stats()
        stats.update(hv=s.hv_passes(), inner_total=s.inner_iterations()[1], k=s.k())
        # behind the run: the public evaluation at every x_k -- the gradient of a run that is not memoised, and the check of the getter's
        for dr in run.dirs[1:]:
            if not memoize:
                dr.g = obj(dr.x).g()
        for x_at, g_got in got:
            assert obj(x_at).g().tobytes() == g_got.tobytes()
    finally:
        s.close()
        obj.close()
    return run, status, stats


_recorded = {}


def _record_once(qn, case):
    """the default run of a case (memoize 1, chunk 8, to convergence), made once for the tests that share it"""
    if case not in _recorded:
        _recorded[case] = record(qn, case)
    return _recorded[case]


def _audited(run, family):
    rep = AU.audit(run)
    print(AU.line(rep))
    w = _worst.setdefault(family, {c: 0.0 for c in AU.CHECKS})
    for c in AU.CHECKS:
        w[c] = max(w[c], rep["worst"][c])
    unlicensed = [(r["k"], r["j"]) for r in rep["rows"] if r["j"] >= 1 and r["ended"] in ("tol", "cap") and not r["licensed"]]
    print(f"    not licensed (k, j_k): {unlicensed}")
    print(f"    worst ratios so far, by family: { {f: {c: float(f'{v:.4g}') for c, v in d.items()} for f, d in _worst.items()} }")
    return rep, unlicensed


# ---- 1. the well-conditioned cases: every direction licensed, every check ----
@pytest.mark.parametrize("case", AU.LSE_CASES + AU.UNSCALED_CASES, ids=str)
def test_every_direction_of_an_unscaled_run(qn, case):
    run, status, _ = _record_once(qn, case)
    rep, unlicensed = _audited(run, case[0])
    assert rep["directions"] >= 5 and not rep["failures"], rep["failures"]
    assert not unlicensed and rep["ties"] == 0, (unlicensed, rep["ties"])


@pytest.mark.parametrize("case", [("lse", 257, 200, "wolfe"), ("logistic", 40, 65, "bt"), ("slogistic", 96, 64, "wolfe"), ("multinomial", 40, 13, 5, "bt"),
                                  ("smultinomial", 96, 16, 4, "wolfe")], ids=str)
def test_a_run_that_is_not_memoised_is_the_same_run(qn, case):
    """memoize 0: the loop top evaluates x_{k+1} again; the directions are the memoised run's bit for bit, and the audit holds them from the public
    evaluation's gradients"""
    run, _, _ = record(qn, case, memoize=0)
    base, _, _ = _record_once(qn, case)
    assert len(run.dirs) == len(base.dirs)
    assert all(p.d.tobytes() == q.d.tobytes() and p.g.tobytes() == q.g.tobytes() and p.x_next.tobytes() == q.x_next.tobytes() for p, q in zip(run.dirs, base.dirs))
    rep, unlicensed = _audited(run, case[0])
    assert not rep["failures"] and not unlicensed, (rep["failures"], unlicensed)


# ---- 2. the badly scaled problems, plain and Jacobi, to convergence ----
@pytest.mark.parametrize("case", AU.PRECOND_CASES, ids=str)
def test_every_direction_of_a_badly_scaled_run(qn, case):
    """(a) and (b) on every direction of runs of up to 43 outer iterations and 2964 inner steps; (c) and (d) on the licensed ones, which include
    every direction of at most 8 inner steps"""
    run, status, stats = _record_once(qn, case)
    rep, unlicensed = _audited(run, "precond " + case[-1])
    print(f"    {status}: {rep['directions']} outer, {stats['inner_total']} inner steps")
    assert status == "ok" and not rep["failures"], rep["failures"]
    assert rep["worst"]["b"] > 0.0 and all(j > 8 for _, j in unlicensed), unlicensed


# ---- 3. the other exits and the other ways to run ----
def test_cap_exits(qn):
    case = ("lse", 96, 64, "bt")
    run, _, _ = record(qn, case, max_inner=2)
    rep, unlicensed = _audited(run, "lse")
    capped = [r for r in rep["rows"] if r["ended"] == "cap"]
    assert capped and all(r["j"] == 2 and r["b"] is None and r["c"] is not None for r in capped)
    assert not rep["failures"] and not unlicensed


def test_negative_curvature_at_the_first_step(qn):
    a, c, _, _ = NC.problem(3, 5)
    run, status, _ = record(qn, ("lse", 3, 5, "bt"), ops=AU.LseOps(a, c, NC.NEG_MU), iters=3, mu=NC.NEG_MU)
    rep, _ = _audited(run, "lse")
    first = rep["rows"][0]
    assert first["ended"] == "negcurv" and first["j"] == 0 and run.dirs[0].d.tobytes() == (-run.dirs[0].g).tobytes()
    assert not rep["failures"]


def test_two_calls_are_audited_as_one(qn):
    case = ("logistic", 96, 64, "bt")
    two, _, _ = record(qn, case, iters=4, calls=2)
    one, _, _ = record(qn, case, iters=8)
    assert len(two.dirs) == 8 and all(p.d.tobytes() == q.d.tobytes() and p.g.tobytes() == q.g.tobytes() for p, q in zip(two.dirs, one.dirs))
    rep, unlicensed = _audited(two, "logistic")
    assert not rep["failures"] and not unlicensed


@pytest.mark.parametrize("chunk", [1, 8])
def test_chunks(qn, chunk):
    """a chunk of 1 puts a peek between any two inner steps, a chunk of 8 a boundary at inner step 8, 16, ...: the directions of 12 and more steps of
    this case cross it"""
    case = ("precond", "dense", 96, 64, "bt", "jacobi")
    run, status, _ = record(qn, case, chunk=chunk) if chunk != 8 else _record_once(qn, case)
    assert all(p.d.tobytes() == q.d.tobytes() for p, q in zip(run.dirs, _record_once(qn, case)[0].dirs))  # (the chunk never changes a bit)
    assert max(d.j for d in run.dirs) > 16
    rep, unlicensed = _audited(run, "precond jacobi")
    assert status == "ok" and not rep["failures"] and all(j > 8 for _, j in unlicensed)


# ---- 4. the two getters ----
def test_the_getters_refuse_what_they_do_not_hold(qn):
    a, c, mu, x0 = NC.problem(96, 64)
    obj = qn.LogSumExp(a, c, mu)
    s = qn.NewtonCG(NC.TOL, x0)
    other = qn.BFGS(1e-7, x0)
    try:
        for getter in (s.direction, s.gradient):  # nothing has run
            with pytest.raises(qn.ErrorInputParams, match="is held"):
                getter()
        with pytest.raises(qn.MaxIterReached):
            s.minimize(qn.BackTracking(1e-4, 0.5), obj, 0, NC.MAX_LS)  # a cap of 0 evaluates nothing
        with pytest.raises(qn.ErrorInputParams, match="cap of 0 evaluates nothing"):
            s.gradient()
        with pytest.raises(qn.MaxIterReached):
            s.minimize(qn.BackTracking(1e-4, 0.5), obj, 2, NC.MAX_LS)
        d, g, x = s.direction(), s.gradient(), s.x()
        assert g.tobytes() == obj(x).g().tobytes() and float(d @ d) > 0.0
        s.set_x(x)  # x set since: the evaluation is no longer the current point's
        with pytest.raises(qn.ErrorInputParams, match="x was set since"):
            s.gradient()
        s.minimize(qn.BackTracking(1e-4, 0.5), obj, NC.ITERS, NC.MAX_LS)  # to convergence: the last loop top searched nothing
        with pytest.raises(qn.ErrorInputParams, match="never searched|no searched direction"):
            s.direction()
        assert s.gradient().tobytes() == obj(s.x()).g().tobytes() and float(np.max(np.abs(s.gradient()))) < NC.TOL
        for getter in (other.direction, other.gradient):
            with pytest.raises(qn.ErrorInputParams, match="vector family"):
                getter()
    finally:
        s.close()
        other.close()
        obj.close()


@pytest.mark.parametrize("method", ["lbfgs", "spg", "cg"])
def test_the_getters_on_the_rest_of_the_vector_family(qn, method):
    """x_{k+1} = fl(x_k + fl(t_k d_k)) bit for bit from the direction read in the callback, and the gradient read there is the objective's at x_{k+1}"""
    a, c, mu, x0 = NC.problem(40, 65)
    obj = qn.LogSumExp(a, c, mu)
    n = x0.size
    s = {"lbfgs": lambda: qn.LBFGS(1e-9, x0), "cg": lambda: qn.NonlinearCG(1e-9, x0),
         "spg": lambda: qn.SpectralProjectedGradient(1e-9, x0, obj, np.full(n, -np.inf), np.full(n, np.inf))}[method]()
    try:
        s.set_trace(6, with_x=True)
        rec = []
        try:
            s.minimize(qn.GLLQuadratic(1e-4, 5) if method == "spg" else qn.BackTracking(1e-4, 0.5), obj, 6, 30,
                       callback=lambda sv: rec.append((sv.x(), sv.direction(), sv.gradient())))
        except qn.MaxIterReached:
            pass
        tr, _ = s.trace()
        assert len(rec) == len(tr) == 6
        x = np.array(x0)
        for r, (x_next, d, g_next) in zip(tr, rec):
            assert x_next.tobytes() == (x + r["t"] * d).tobytes()
            x = x_next
        for x_next, _, g_next in rec:
            assert obj(x_next).g().tobytes() == g_next.tobytes()
    finally:
        s.close()
        obj.close()
