"""Measures nonlinear conjugate gradient (QN_NONLINEAR_CG, csrc/qn_cg.hip.h) beside LBFGS(m = 5), both with StrongWolfe(1e-4, 0.1).  Not run by any test.

Objectives: SparseQuadratic on the 2-D five-point Laplacian plus a shift of 0.05 at n = 2^20, 2^22, 2^24 (tools/bench_sparse.py's), LogSumExp with a
64 x n matrix, and the example device closure (examples/device_closure.hip, the double-well chain).  One JSON line per (objective, n, solver) with
  * ms per iteration (wall clock over a whole qn_minimize call), iterations and oracle evaluations until ||g||_inf < --gnorm (or the cap), restarts;
  * from ONE profiled call that continues a warm-up of 3 iterations: microseconds per launch and bytes/s of
      NonlinearCG  cg_dir_kernel (t_hpass_ms; 16 n read + 16 n written = 32 n bytes; a launch on the -g branch reads 8 n less, so a run with
                   restarts overstates its rate: `restarts` is on the line) and cg_accept_kernel (t_hreduce_ms; 32 n read + 16 n written = 48 n)
      LBFGS        vec_dir_kernel in phase NSOLVE (t_ereduce_ms; x, g, z, lb, ub read, d written = 48 n) -- cg_dir_kernel's neighbour per byte
    each minus the fixed part of an event bracket (Context.event_bracket_overhead_ms).
Profiling mode has no class of its own for lbfgs_accept_kernel and vec_accept_kernel (both are timed with the one-workgroup kernels, t_ctl_ms):
their per-launch averages, beside cg_accept_kernel's, come from a kernel trace of the same run in a run of its own,
    rocprofv3 --kernel-trace --stats -- python tools/bench_cg.py --no-profile --solvers hz lbfgs spg
(`spg`: SpectralProjectedGradient + GLLQuadratic, the method that launches vec_accept_kernel: 32 n read (x, d, g, gt) + 16 n written, as
lbfgs_accept_kernel is 32 n read + 32 n written).

    python tools/bench_cg.py [--sizes 20 22 24] [--objectives lap lse chain] [--solvers fr pr+ hs+ dy hz lbfgs] [--iters 200] [--gnorm 1e-6] [--no-profile]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CG = ("fr", "pr+", "hs+", "dy", "hz")


def _minimize(qn, s, ls, oracle, iters):
    t0 = time.perf_counter()
    try:
        s.minimize(ls, oracle, iters, 50)
        status = "ok"
    except qn.MaxIterReached:
        status = "max_iter"
    except qn.SolverError as e:  # (a search that cannot go on at f's last bits: reported, not fatal)
        status = type(e).__name__
    qn.default_context().synchronize()
    return status, time.perf_counter() - t0


def _make(qn, solver, gnorm, x0):
    if solver in CG:
        return qn.NonlinearCG(gnorm, x0, variant=solver, memoize=1), qn.StrongWolfe(1e-4, 0.1)
    if solver == "lbfgs":
        return qn.LBFGS(gnorm, x0, m=5, memoize=1), qn.StrongWolfe(1e-4, 0.1)
    raise ValueError(solver)


def _run(qn, solver, oracle, x0, iters, gnorm):
    if solver == "spg":
        n = x0.size
        s, ls = qn.SpectralProjectedGradient(gnorm, x0, oracle, np.full(n, -np.inf), np.full(n, np.inf), memoize=1), qn.GLLQuadratic(1e-4, 10)
    else:
        s, ls = _make(qn, solver, gnorm, x0)
    s.set_trace(iters)
    status, dt = _minimize(qn, s, ls, oracle, iters)
    tr, _ = s.trace()
    st = s.stats()
    out = dict(status=status, iterations=len(tr), oracle_evals=st["oracle_evals"], ms_per_iter=1e3 * dt / max(1, len(tr)),
               gnorm_last=tr[-1]["gnorm"] if tr else None, host_syncs=st["host_syncs"])
    if solver in CG:
        out["restarts"] = s.restarts()
    s.close()
    return out


def _profile(qn, solver, oracle, x0, iters, bracket_ms):
    """per-launch figures: 3 iterations unprofiled, then one profiled call that continues them"""
    s, ls = _make(qn, solver, 0.0, x0)
    _minimize(qn, s, ls, oracle, 3)
    before = s.stats()
    s.set_profiling(1)
    _minimize(qn, s, ls, oracle, iters)
    st = s.stats()
    s.close()
    n = x0.size
    kernels = (("cg_dir", "hpass", 32 * n), ("cg_accept", "hreduce", 48 * n)) if solver in CG else (("vec_dir", "ereduce", 48 * n),)
    out = {}
    for name, cls, nbytes in kernels:
        cnt = st[f"n_{cls}_timed"] - before[f"n_{cls}_timed"]
        us = 1e3 * ((st[f"t_{cls}_ms"] - before[f"t_{cls}_ms"]) / cnt - bracket_ms) if cnt else None
        out[f"{name}_us"], out[f"{name}_launches_timed"] = us, cnt
        out[f"{name}_tb_per_s"] = nbytes / (us * 1e-6) / 1e12 if us and us > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[20, 22, 24])
    ap.add_argument("--objectives", nargs="*", default=["lap", "lse", "chain"])
    ap.add_argument("--solvers", nargs="*", default=list(CG) + ["lbfgs"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--profile-iters", type=int, default=20)
    ap.add_argument("--gnorm", type=float, default=1e-6)
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    qn = ge.load_package()
    bracket_ms = qn.default_context().event_bracket_overhead_ms()
    for lg in a.sizes:
        n = 1 << lg
        rng = np.random.default_rng(5)
        for objective in a.objectives:
            if objective == "lap":
                import bench_sparse as BS
                indptr, cols, vals = BS.laplacian(1 << (lg // 2))
                x0 = np.zeros(n)
                obj = qn.SparseQuadratic(indptr, cols, vals, np.ones(n))
                oracle, closer = obj, obj.close
            elif objective == "chain":
                from test_gpu_device_closure import _Chain
                x0 = rng.uniform(-2.0, 2.0, n)
                ch = _Chain(qn, rng.uniform(0.5, 2.0, n), 0.3)
                oracle, closer = ch.closure, ch.close
            else:
                x0 = rng.standard_normal(n) / np.sqrt(n)
                obj = qn.LogSumExp(rng.standard_normal((64, n)), rng.standard_normal(64), 0.5)
                oracle, closer = obj, (lambda: None)
            for solver in a.solvers:
                line = dict(n=n, objective=objective, solver=solver, gnorm=a.gnorm)
                line.update(_run(qn, solver, oracle, x0, a.iters, a.gnorm))
                if not a.no_profile and solver != "spg":
                    line.update(_profile(qn, solver, oracle, x0, a.profile_iters, bracket_ms))
                print(json.dumps(line), flush=True)
            closer()


if __name__ == "__main__":
    main()
