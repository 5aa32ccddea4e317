"""Measures limited-memory BFGS (QN_LBFGS, csrc/qn_lbfgs.hip.h) beside SpectralProjectedGradient with the same line search.  Not run by any test.

For m = 5 and 17 at n = 2^20, 2^22, 2^24, on the example device closure (examples/device_closure.hip, the double-well chain) and on LogSumExp
with a 64 x n matrix, GLLQuadratic(1e-4, 10) for both solvers:
  * ms per iteration (wall clock over a whole qn_minimize call) of L-BFGS and of SPG;
  * iterations until ||projected gradient||_inf < --gnorm (or the cap);
  * from ONE profiled L-BFGS call that continues a warm-up of m + 2 iterations (so every timed launch sees the memory as the line reports it:
    `stored_pairs`, `resets`): microseconds per launch and bytes/s of lbfgs_gram_kernel, of lbfgs_apply_kernel and of vec_dir_kernel on the same
    vectors.  Profiling mode times the three apart (t_hpass_ms, t_hreduce_ms, t_ereduce_ms: include/qn_hip.h).  Bytes, k = stored pairs:
    Gram (2 k + 1) 8 n algorithmic (the line also gives the traffic the kernel issues, (2 k + 3 ceil(k / 4)) 8 n: g, s_p, y_p once per group of 4
    pairs), apply (2 k + 2) 8 n, vec_dir_kernel in phase NSOLVE 6 x 8 n (x, g, z, lb, ub read, d written).

    python tools/bench_lbfgs.py [--sizes 20 22 24] [--memories 5 17] [--iters 40] [--gnorm 1e-6] [--objectives chain lse]
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


def _minimize(qn, s, ls, oracle, iters):
    t0 = time.perf_counter()
    try:
        s.minimize(ls, oracle, iters, 50)
        status = "ok"
    except qn.MaxIterReached:
        status = "max_iter"
    qn.default_context().synchronize()
    return status, time.perf_counter() - t0


def _run(qn, make, oracle, ls, iters):
    s = make()
    s.set_trace(iters)
    status, dt = _minimize(qn, s, ls, oracle, iters)
    tr, _ = s.trace()
    s.close()
    return dict(status=status, iterations=len(tr), ms_per_iter=1e3 * dt / max(1, len(tr)), gnorm_last=tr[-1]["gnorm"] if tr else None)


def _profile(qn, make, oracle, ls, m, iters, n):
    """per-launch figures at a warmed-up memory: m + 2 iterations unprofiled, then one profiled call that continues them"""
    s = make()
    _minimize(qn, s, ls, oracle, m + 2)
    before = s.stats()
    s.set_profiling(1)
    _minimize(qn, s, ls, oracle, iters)
    st = s.stats()
    k, resets = s.stored_pairs(), s.resets()
    s.close()
    out = dict(stored_pairs=k, resets=resets)
    groups = (k + 3) // 4
    for name, cls, nbytes in (("gram", "hpass", (2 * k + 1) * 8 * n), ("apply", "hreduce", (2 * k + 2) * 8 * n), ("vec_dir", "ereduce", 6 * 8 * n)):
        cnt = st[f"n_{cls}_timed"] - before[f"n_{cls}_timed"]
        ms = st[f"t_{cls}_ms"] - before[f"t_{cls}_ms"]
        us = 1e3 * ms / cnt if cnt else None
        out[f"{name}_us"] = us
        out[f"{name}_launches_timed"] = cnt
        out[f"{name}_tb_per_s"] = nbytes / (us * 1e-6) / 1e12 if us else None
    if out["gram_us"]:
        out["gram_issued_tb_per_s"] = (2 * k + 3 * groups) * 8 * n / (out["gram_us"] * 1e-6) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[20, 22, 24])
    ap.add_argument("--memories", type=int, nargs="*", default=[5, 17])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--gnorm", type=float, default=1e-6)
    ap.add_argument("--objectives", nargs="*", default=["chain", "lse"])
    a = ap.parse_args()
    import __graft_entry__ as ge
    qn = ge.load_package()
    for lg in a.sizes:
        n = 1 << lg
        rng = np.random.default_rng(5)
        lb, ub = np.full(n, -np.inf), np.full(n, np.inf)
        for objective in a.objectives:
            if objective == "chain":
                from test_gpu_device_closure import _Chain
                x0 = rng.uniform(-2.0, 2.0, n)
                ch = _Chain(qn, rng.uniform(0.5, 2.0, n), 0.3)
                oracle, closer = ch.closure, ch.close
            else:
                x0 = rng.standard_normal(n) / np.sqrt(n)
                obj = qn.LogSumExp(rng.standard_normal((64, n)), rng.standard_normal(64), 0.5)
                oracle, closer = obj, (lambda: None)
            ls = qn.GLLQuadratic(1e-4, 10)
            spg = _run(qn, lambda: qn.SpectralProjectedGradient(a.gnorm, x0, oracle, lb, ub, memoize=1), oracle, ls, a.iters)
            for m in a.memories:
                run = _run(qn, lambda: qn.LBFGS(a.gnorm, x0, m=m, memoize=1), oracle, ls, a.iters)
                line = dict(n=n, objective=objective, m=m, lbfgs_ms_per_iter=run["ms_per_iter"], spg_ms_per_iter=spg["ms_per_iter"],
                            lbfgs_iterations=run["iterations"], spg_iterations=spg["iterations"], lbfgs_status=run["status"],
                            spg_status=spg["status"], lbfgs_gnorm_last=run["gnorm_last"], spg_gnorm_last=spg["gnorm_last"])
                line.update(_profile(qn, lambda: qn.LBFGS(a.gnorm, x0, m=m, memoize=1), oracle, ls, m, a.iters, n))
                print(json.dumps(line), flush=True)
            closer()


if __name__ == "__main__":
    main()
