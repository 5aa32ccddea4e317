"""GPU tests of QN_NEWTON_CG (NewtonCG; kernels csrc/qn_newton_cg.hip.h and qn_lse_hv.hip.h, pump csrc/qn_host_vec.hip.h) against the restatement
tests/ref_newton_cg.py inside the windows tests/test_ref_newton_cg.py licenses: x at 1e-9 max(1, ||x||) plus every decision -- t, n_evals, the inner
count j_k (read in the callback), the negative-curvature and fallback counts --, with memoize 0 and 1 and chunks of 1, 3 and 8 inner steps, which
never change a bit; convergence, the synchronisation budget, the cap, negative curvature, warm restarts, determinism, error paths, the C++ example."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import newton_cg_cases as NC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _ls(qn, kind):
    return qn.StrongWolfe(*NC.WOLFE) if kind == "wolfe" else qn.BackTracking(1e-4, 0.5)


def gpu_run(qn, m, n, ls, iters=NC.ITERS, memoize=1, chunk=8, mu=None, max_inner=0, calls=1, tol=NC.TOL):
    """one NewtonCG run (`calls` successive minimize calls of `iters` iterations): everything the tests compare"""
    a, c, mu0, x0 = NC.problem(m, n)
    obj = qn.LogSumExp(a, c, mu0 if mu is None else mu)
    s = qn.NewtonCG(tol, x0, max_inner=max_inner, chunk=chunk, memoize=memoize)
    out = dict(trace=[], xs=[], inner=[], neg=[], fb=[], syncs=0, hv=0, inner_total=0, status="ok", k=0, obj_bytes=0, path=0)
    try:
        for _ in range(calls):
            s.set_trace(iters, with_x=True)
            rec = []
            try:
                s.minimize(_ls(qn, ls), obj, iters, NC.MAX_LS, callback=lambda sv: rec.append((sv.inner_iterations()[0], sv.negative_curvature(), sv.fallbacks())))
                out["status"] = "ok"
            except qn.MaxIterReached:
                out["status"] = "max_iter"
            tr, xs = s.trace()
            st = s.stats()
            out["trace"] += list(tr)
            out["xs"] += [np.array(x) for x in xs]
            out["inner"] += [r[0] for r in rec]
            out["neg"] += [r[1] for r in rec]
            out["fb"] += [r[2] for r in rec]
            out["syncs"] += st["host_syncs"]
            out["hv"] += s.hv_passes()
            out["inner_total"] += s.inner_iterations()[1]
            out["k"] += s.k()
            out["obj_bytes"], out["path"] = st["obj_bytes"], st["path"]
        out["x"] = s.x()
    finally:
        s.close()
        obj.close()
    return out


def _bits(run):
    return (run["x"].tobytes(), [x.tobytes() for x in run["xs"]], [(r["t"], r["n_evals"], r["f"]) for r in run["trace"]], run["inner"], run["status"])


_runs = {}


def _run(qn, m, n, ls, memoize, chunk):
    key = (m, n, ls, memoize, chunk)
    if key not in _runs:
        _runs[key] = gpu_run(qn, m, n, ls, memoize=memoize, chunk=chunk)
    return _runs[key]


# ---- 1. against the restatement, inside the licensed windows ----
@pytest.mark.parametrize("memoize", [1, 0])
@pytest.mark.parametrize("m,n,ls", NC.CASES)
def test_against_the_restatement(qn, m, n, ls, memoize):
    w = NC.window(m, n, ls)
    ref = NC.ref_case(m, n, ls)[0]
    run = _run(qn, m, n, ls, memoize, 8)
    assert len(run["trace"]) >= w and len(run["inner"]) == len(run["trace"])
    worst = 0.0
    for k in range(w):
        r, g = ref.trace[k], run["trace"][k]
        dx = float(np.linalg.norm(run["xs"][k] - ref.trace_x[k]) / max(1.0, np.linalg.norm(ref.trace_x[k])))
        worst = max(worst, dx)
        assert dx <= NC.GPU_TOL, (k, dx)
        assert g["n_evals"] == r["n_evals"], (k, g, r)
        assert (g["t"] == r["t"]) if ls == "bt" else (abs(g["t"] - r["t"]) <= NC.GPU_TOL * abs(r["t"])), (k, g["t"], r["t"])
        assert run["inner"][k] == ref.inner[k], (k, run["inner"], ref.inner)
    assert run["neg"][w - 1] == 0 and run["fb"][w - 1] == 0 and set(ref.why[:w]) == {"tol"}
    print(f"NewtonCG {(m, n, ls)} memoize={memoize}: window {w} of {len(ref.trace)}, worst |x - x_ref| = {worst:.2e}, GPU k = {run['k']} ({run['status']})")


@pytest.mark.parametrize("m,n,ls", [(96, 64, "bt"), (257, 200, "wolfe"), (5, 2050, "bt")])
def test_the_chunk_never_changes_a_bit(qn, m, n, ls):
    base = _bits(_run(qn, m, n, ls, 1, 8))
    for chunk in (1, 3):
        assert _bits(_run(qn, m, n, ls, 1, chunk)) == base, chunk
    assert _bits(_run(qn, m, n, ls, 0, 8)) == base  # (and memoize 0 evaluates the accepted point again: the same bits)


# ---- 2. convergence, the synchronisation budget, the counters ----
@pytest.mark.parametrize("m,n", NC.CONVERGENCE)
def test_convergence_and_the_sync_budget(qn, m, n):
    ref, _, ref_status = NC.ref_case(m, n, "bt")
    assert ref_status == "ok"
    for chunk in (8, 3):
        run = _run(qn, m, n, "bt", 1, chunk)
        assert run["status"] == "ok" and run["k"] <= 1.5 * ref.k, (run["k"], ref.k)
        a, c, mu, _ = NC.problem(m, n)
        al, xl = a.astype(LD), run["x"].astype(LD)
        z = al @ xl + c.astype(LD)
        e = np.exp(z - z.max())
        g = al.T @ (e / e.sum()) + LD(mu) * xl
        assert float(np.max(np.abs(g))) < NC.TOL
        assert run["hv"] == run["inner_total"] == sum(run["inner"])
        extra_trials = sum(r["ls_iters"] - 1 for r in run["trace"])
        budget = sum(max(1, math.ceil(j / chunk)) for j in run["inner"]) + extra_trials + 2
        print(f"NewtonCG ({m}, {n}) chunk={chunk}: k={run['k']} (restatement {ref.k}) inner={run['inner']} host_syncs={run['syncs']} budget={budget}")
        assert run["syncs"] <= budget, (run["syncs"], budget)
        assert run["obj_bytes"] % (8 * m) == 0 and run["obj_bytes"] >= 8 * m * n * (run["hv"] + 2 * run["k"])  # (n_pad >= n; one weights pass per iteration)
        assert run["path"] & qn._abi.PATH_NEWTON_CG and run["path"] & qn._abi.PATH_VECTOR


def test_max_inner_caps_the_loop(qn):
    ref = NC.run_ref(96, 64, "bt", max_inner=2)[0]
    run = gpu_run(qn, 96, 64, "bt", max_inner=2)
    assert max(run["inner"]) == 2 and all(j <= 2 for j in run["inner"])
    w = min(6, len(ref.trace), len(run["trace"]))
    assert run["inner"][:w] == ref.inner[:w] and "cap" in ref.why[:w]
    for k in range(w):
        assert np.linalg.norm(run["xs"][k] - ref.trace_x[k]) <= NC.GPU_TOL * max(1.0, np.linalg.norm(ref.trace_x[k]))


def test_negative_curvature_takes_the_gradient(qn):
    ref = NC.run_ref(3, 5, "bt", iters=3, mu=NC.NEG_MU)[0]
    assert ref.why[0] == "negcurv" and ref.inner[0] == 0
    run = gpu_run(qn, 3, 5, "bt", iters=3, mu=NC.NEG_MU)
    assert run["status"] == "max_iter" and run["neg"][0] >= 1 and run["inner"][0] == 0
    a, c, _, x0 = NC.problem(3, 5)
    g0 = NC.S.lse_fn(a, c, NC.NEG_MU)(x0)[1]
    t0 = run["trace"][0]["t"]
    assert np.linalg.norm(run["xs"][0] - (x0 + t0 * -g0)) <= NC.GPU_TOL * max(1.0, np.linalg.norm(x0))  # d = -g
    for k in range(3):
        assert run["inner"][k] == ref.inner[k] and run["trace"][k]["t"] == ref.trace[k]["t"] and run["trace"][k]["n_evals"] == ref.trace[k]["n_evals"], k
    assert run["neg"][2] == ref.neg_curv and run["fb"][2] == ref.fallbacks


# ---- 3. warm restarts, determinism ----
def test_two_calls_are_one(qn):
    one = gpu_run(qn, 96, 64, "bt", iters=8)
    two = gpu_run(qn, 96, 64, "bt", iters=4, calls=2)
    assert one["x"].tobytes() == two["x"].tobytes() and one["inner"] == two["inner"]
    assert [x.tobytes() for x in one["xs"]] == [x.tobytes() for x in two["xs"]]


def test_determinism_across_runs(qn):
    assert _bits(gpu_run(qn, 257, 200, "wolfe")) == _bits(_run(qn, 257, 200, "wolfe", 1, 8))


# ---- 4. error paths ----
def test_error_paths(qn):
    a, c, mu, x0 = NC.problem(3, 5)
    lse = qn.LogSumExp(a, c, mu)
    quad = qn.Quadratic(np.eye(5), np.zeros(5))
    sp = qn.SparseQuadratic(np.arange(6), np.arange(5), np.ones(5), np.zeros(5))
    bt = qn.BackTracking(1e-4, 0.5)
    try:
        s = qn.NewtonCG(1e-7, x0)
        fn = NC.S.lse_fn(a, c, mu)
        with pytest.raises(qn.ErrorInputParams, match="closure"):
            s.minimize(bt, lambda x: fn(x), 5, 5)
        with pytest.raises(qn.ErrorInputParams, match="LogSumExp"):
            s.minimize(bt, quad, 5, 5)
        with pytest.raises(qn.ErrorInputParams, match="LogSumExp"):
            s.minimize(bt, sp, 5, 5)
        with pytest.raises(qn.ErrorInputParams, match="BackTracking or StrongWolfe"):
            s.minimize(qn.GLLQuadratic(1e-4, 10), lse, 5, 5)
        with pytest.raises(qn.ErrorInputParams, match="BackTracking or StrongWolfe"):
            s.minimize(qn.MoreThuente(), lse, 5, 5)
        with pytest.raises(qn.ErrorInputParams, match="unbounded"):
            s.minimize(qn.StrongWolfe().with_lower_bound(np.full(5, -1.0)), lse, 5, 5)
        lb, ub = np.full(5, -1.0), np.full(5, 1.0)
        dp = C.POINTER(C.c_double)
        with pytest.raises(qn.ErrorInputParams, match="unbounded"):
            qn.solver._check(qn._abi.lib().qn_solver_set_bounds(s.h, lb.ctypes.data_as(dp), ub.ctypes.data_as(dp)))
        for bad in (0.0, 1.0, -0.1, float("nan")):
            with pytest.raises(qn.ErrorInputParams, match="eta_max"):
                s.set_newton_cg(eta_max=bad)
        with pytest.raises(qn.ErrorInputParams, match="chunk"):
            s.set_newton_cg(chunk=0)
        s.close()
        other = qn.NonlinearCG(1e-7, x0)
        with pytest.raises(qn.ErrorInputParams, match="NewtonCG"):
            qn.solver._check(qn._abi.lib().qn_solver_set_newton_cg(other.h, 0.5, 0, 8))
        with pytest.raises(qn.ErrorInputParams, match="NewtonCG"):
            qn.solver._check(qn._abi.lib().qn_solver_newton_cg_state(other.h, None, None, None, None, None))
        other.close()
    finally:
        lse.close()
        quad.close()
        sp.close()


def test_examples_newton_cg_cpp():
    exe = os.path.join(ROOT, "examples", "newton_cg_example.bin")
    assert os.path.exists(exe), "examples/newton_cg_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "outer iterations" in p.stdout and "inner steps" in p.stdout and p.stdout.strip().endswith("newton cg example ok")
