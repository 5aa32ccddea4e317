"""Every iteration of GPU runs of SpectralProjectedGradient, ProjectedGradientDescent, ProjectedNewton and SpectralProjectedNewton with GLLQuadratic,
BackTracking and BackTrackingB (kernels vec_dir, vec_top, vec_trial, vec_decide, vec_accept, vec_post and pn_small of csrc/qn_vec.hip.h) replayed
step by step from the run's own records: tests/vec_replay.py, where the equalities and the bounds are stated; cases and their conditions in
tests/vec_replay_cases.py, licensed on the CPU by tests/test_ref_vec_replay.py.  The closures are host closures that record every point they are
asked, in order, so directions, trial points, iterates and counts are compared bit for bit and only the dot products inside derived rounding
bounds.  The cap is the CPU's: no skipped iteration, no undecidable decision.  The last test prints the worst ratio per quantity and size."""
import numpy as np
import pytest

import lbfgs_replay as LR
import vec_replay as VR
import vec_replay_cases as C

pytestmark = pytest.mark.gpu
PATH_VECTOR = 64
_RUNS, _TALLY = {}, {}


def gpu_run(qn, case, callback=True):
    fn, x0, lb, ub = C.problem(case)
    method, spectral, newton = case["method"], case["method"] in ("spg", "spn"), case["method"] in ("pn", "spn")
    limited = case.get("limited", False)
    spec = C.line_search(case, lb, ub, fn)
    rec = obj = None
    if limited:  # the device objective of the same function
        oracle = obj = qn.SparseQuadratic(*fn.csr, fn.b)
    else:
        class Eval(qn.FuncEvalMultivariate):  # the closure's FuncEval; reading its Hessian marks the call as the solver's Hessian callback
            def hessian(self):
                self.read()
                return super().hessian()

        def wrap(f, g, h, read):
            e = Eval(f, g).with_hessian(h)
            e.read = read
            return e
        oracle = rec = VR.HRecorder(fn, wrap) if newton else LR.Recorder(lambda x: fn(x)[:2], keep_x=True)
    lmin, lmax = case.get("lambdas", (1e-3, 1e3))
    run = VR.Run(method, spec, lb, ub, x0, rec, case["memoize"], case["max_ls"], case["tol"], lmin, lmax, limited=limited)
    run.hessian_calls = newton
    cls = {"spg": qn.SpectralProjectedGradient, "pgd": qn.ProjectedGradientDescent, "pn": qn.ProjectedNewton, "spn": qn.SpectralProjectedNewton}[method]
    if spectral:
        s = cls(case["tol"], x0, oracle, lb, ub, memoize=case["memoize"])
        run.lam0 = s.lambda_()
        s.with_lambdas(lmin, lmax)
    else:
        s = cls(case["tol"], x0, lb, ub)
        s.memoize = case["memoize"]
    if spec["kind"] == "gll":
        ls = qn.GLLQuadratic(spec["c1"], spec["m"]).with_sigmas(spec["sigma1"], spec["sigma2"])
    elif spec["kind"] == "bt":
        ls = qn.BackTracking(spec["c1"], spec["beta"])
    else:
        ls = qn.BackTrackingB(spec["c1"], spec["beta"], spec["lo"], spec["hi"])
    if limited:
        run.grads.append(s.gradient())  # the constructor's evaluation at P(x0), as the device holds it
    for iters in case["plan"]:
        s.set_trace(iters, with_x=True)
        seen = []

        def cb(r):
            seen.append(dict(d=r.direction(), lam=r.lambda_() if spectral else None, s_norm=r.s_norm() if method == "pn" else None,
                             y_norm=r.y_norm() if method == "pn" else None))
            if limited:
                run.grads.append(r.gradient())
        converged = True
        try:
            s.minimize(ls, oracle, iters, case["max_ls"], callback=cb if callback else None)
        except qn.MaxIterReached:
            converged = False
        tr, xs = s.trace()
        st = s.stats()
        assert st["path"] & PATH_VECTOR
        if not callback:
            seen = [dict(d=None, lam=None, s_norm=None, y_norm=None) for _ in tr]
        run.add_call(tr, list(xs), seen, st["oracle_calls"], st["oracle_evals"], converged)
    if run.calls[-1]["its"]:
        assert np.array_equal(s.x(), run.calls[-1]["its"][-1]["x"])
    s.close()
    if obj is not None:
        obj.close()
    return run


def _run(qn, case):
    if case["name"] not in _RUNS:
        _RUNS[case["name"]] = gpu_run(qn, case)
    return _RUNS[case["name"]]


def _x_trace(run):
    return b"".join(it["x"].tobytes() for c in run.calls for it in c["its"])


@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_replay(qn, case):
    rep = VR.replay(_run(qn, case))
    for q, v in rep.worst.items():
        key = (q, case["n"])
        _TALLY[key] = max(_TALLY.get(key, 0.0), v)
    VR.check(rep, case["name"])
    C.check_conditions(case, rep)


def test_call_plans_give_one_trace(qn):
    group = [c for c in C.CASES if c.get("group") == "plan"]
    assert [c["plan"] for c in group] == [(6,), (3, 3), (1, 2, 3)]
    traces = [_x_trace(_run(qn, c)) for c in group]
    assert traces[0] == traces[1] == traces[2]


@pytest.mark.parametrize("name", ["spg-gll-chain-2049", "pgd-btb-crafted-2049", "pn-gll-quartic-17"])
def test_a_callback_changes_nothing(qn, name):
    case = next(c for c in C.CASES if c["name"] == name)
    assert _x_trace(gpu_run(qn, case, callback=False)) == _x_trace(_run(qn, case))


def test_tally():
    """the record (not a tolerance): the worst ratio per quantity and per size over the cases run in this session"""
    sizes = sorted({n for _, n in _TALLY})
    for q in VR.Report.QUANTITIES:
        row = [(n, _TALLY[(q, n)]) for n in sizes if _TALLY.get((q, n), 0.0) > 0.0]
        print(f"vec replay tally {q:9s} " + (", ".join(f"{n}: {v:.2e}" for n, v in row) or "exact at every size"))
