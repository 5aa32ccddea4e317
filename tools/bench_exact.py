"""Measures the ExactQuadratic line search (QN_LS_EXACT_QUADRATIC, csrc/qn_vec_exact.hip.h) beside StrongWolfe(1e-4, 0.1) on the 2-D five-point
Laplacian plus a shift of 0.05 at n = 2^20, 2^22, 2^24 (tools/bench_sparse.py's matrix, b = 1, x0 = 0).  Not run by any test.

One JSON line per (n, configuration) -- "cg-exact0" NonlinearCG(fr) + ExactQuadratic(0), "cg-exact50" ... ExactQuadratic(50), "cg-wolfe" NonlinearCG(fr)
+ StrongWolfe, "lbfgs-wolfe" LBFGS(5) + StrongWolfe -- with
  * status, iterations, matrix passes (evaluations by the objective + curvature passes) and milliseconds (wall clock over the whole qn_minimize call)
    until ||g||_inf < --gnorm, or the state at the cap;
  * from ONE profiled call that continues a warm-up of 3 iterations, microseconds per launch, each minus the fixed part of an event bracket:
      cg-exact50   spq_curv_kernel (t_newton_ms: the profiling class no method of this family uses; 12 nnz + 4 (n + 1) + 16 n bytes) beside
                   spq_eval_kernel (t_eval_ms; 8 n bytes more) -- refresh_every = 2 in that call, so that both kernels run in it --, and
                   exact_advance_kernel (t_ereduce_ms; 32 n read + 16 n written) beside cg_accept_kernel (t_hreduce_ms; the same 48 n bytes)

    python tools/bench_exact.py [--sizes 20 22 24] [--iters 2000] [--gnorm 1e-6] [--no-profile]
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

CONFIGS = ("cg-exact0", "cg-exact50", "cg-wolfe", "lbfgs-wolfe")


def _make(qn, config, gnorm, x0):
    if config == "cg-exact0":
        return qn.NonlinearCG(gnorm, x0, variant="fr"), qn.ExactQuadratic(0)
    if config == "cg-exact50":
        return qn.NonlinearCG(gnorm, x0, variant="fr"), qn.ExactQuadratic(50)
    if config == "cg-wolfe":
        return qn.NonlinearCG(gnorm, x0, variant="fr", memoize=1), qn.StrongWolfe(1e-4, 0.1)
    return qn.LBFGS(gnorm, x0, m=5, memoize=1), qn.StrongWolfe(1e-4, 0.1)


def _minimize(qn, s, ls, obj, iters):
    t0 = time.perf_counter()
    try:
        s.minimize(ls, obj, iters, 50)
        status = "ok"
    except qn.MaxIterReached:
        status = "max_iter"
    except qn.SolverError as e:
        status = type(e).__name__
    qn.default_context().synchronize()
    return status, time.perf_counter() - t0


def _run(qn, config, obj, x0, iters, gnorm):
    s, ls = _make(qn, config, gnorm, x0)
    s.set_trace(iters)
    status, dt = _minimize(qn, s, ls, obj, iters)
    tr, _ = s.trace()
    st, ex = s.stats(), s.exact_state()
    out = dict(status=status, iterations=len(tr), oracle_evals=st["oracle_evals"], curvature_passes=ex["curvature_passes"] if "exact" in config else 0,
               refreshes=ex["refreshes"] if "exact" in config else None, ms=1e3 * dt, gnorm_last=tr[-1]["gnorm"] if tr else None, host_syncs=st["host_syncs"])
    out["matrix_passes"] = out["oracle_evals"] + out["curvature_passes"]
    s.close()
    return out


def _profile(qn, obj, x0, iters, bracket_ms):
    s, ls = qn.NonlinearCG(0.0, x0, variant="fr"), qn.ExactQuadratic(2)
    _minimize(qn, s, ls, obj, 3)
    before = s.stats()
    s.set_profiling(1)
    _minimize(qn, s, ls, obj, iters)
    st = s.stats()
    s.close()
    n = x0.size
    curv = 12 * obj.nnz + 4 * (n + 1) + 16 * n
    out = {}
    for name, cls, nbytes in (("spq_curv", "newton", curv), ("spq_eval", "eval", curv + 8 * n), ("exact_advance", "ereduce", 48 * n), ("cg_accept", "hreduce", 48 * n)):
        cnt = st[f"n_{cls}_timed"] - before[f"n_{cls}_timed"]
        us = 1e3 * ((st[f"t_{cls}_ms"] - before[f"t_{cls}_ms"]) / cnt - bracket_ms) if cnt else None
        out[f"{name}_us"], out[f"{name}_launches_timed"] = us, cnt
        out[f"{name}_tb_per_s"] = nbytes / (us * 1e-6) / 1e12 if us and us > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[20, 22, 24])
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--wolfe-iters", type=int, default=200)
    ap.add_argument("--profile-iters", type=int, default=20)
    ap.add_argument("--gnorm", type=float, default=1e-6)
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    qn = ge.load_package()
    import bench_sparse as BS
    bracket_ms = qn.default_context().event_bracket_overhead_ms()
    for lg in a.sizes:
        n = 1 << lg
        indptr, cols, vals = BS.laplacian(1 << (lg // 2))
        x0 = np.zeros(n)
        obj = qn.SparseQuadratic(indptr, cols, vals, np.ones(n))
        for config in a.configs:
            line = dict(n=n, config=config, gnorm=a.gnorm)
            line.update(_run(qn, config, obj, x0, a.iters if "exact" in config else a.wolfe_iters, a.gnorm))
            if config == "cg-exact50" and not a.no_profile:
                line.update(_profile(qn, obj, x0, a.profile_iters, bracket_ms))
            print(json.dumps(line), flush=True)
        obj.close()


if __name__ == "__main__":
    main()
