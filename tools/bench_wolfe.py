"""Measures L-BFGS with the StrongWolfe line search (QN_LS_STRONG_WOLFE, csrc/qn_vec_wolfe.hip.h) beside L-BFGS with BackTracking(1e-4, 0.5).  Not run
by any test; a record, not a pass criterion.

For m = 5 at n = 2^20 and 2^22, on the example device closure (examples/device_closure.hip, the double-well chain) and on LogSumExp with a
64 x n matrix, memoize = 1, one JSON line per (n, objective) with, for each search:
  * iterations and oracle evaluations until ||projected gradient||_inf < --gnorm (or the cap), and the last norm;
  * pairs rejected (trace records with updated = 0) and resets of the memory;
  * ms per iteration (wall clock over the whole qn_minimize call) and line-search trials per iteration.
NOT MEASURED HERE: wolfe_phi_kernel's own bytes/s (16 n bytes per trial).  Profiling mode times the vector machine's small kernels as one class
(t_ctl_ms), so the figure needs a kernel trace of this script (one kernel-trace run of a profiler around it), which the tool does not start itself.

    python tools/bench_wolfe.py [--sizes 20 22] [--memory 5] [--iters 60] [--gnorm 1e-6] [--objectives chain lse]
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


def _run(qn, x0, m, gnorm, ls, oracle, iters):
    s = qn.LBFGS(gnorm, x0, m=m, memoize=1)
    s.set_trace(iters)
    t0 = time.perf_counter()
    try:
        s.minimize(ls, oracle, iters, 50)
        status = "ok"
    except qn.MaxIterReached:
        status = "max_iter"
    except qn.AbnormalTermination as e:
        status = "abnormal: " + str(e)[:60]
    qn.default_context().synchronize()
    dt = time.perf_counter() - t0
    tr, _ = s.trace()
    st = s.stats()
    out = dict(status=status, iterations=len(tr), oracle_evals=st["oracle_evals"], pairs_rejected=sum(1 for r in tr if not r["updated"]),
               resets=s.resets(), ms_per_iter=1e3 * dt / max(1, len(tr)), trials_per_iter=sum(r["ls_iters"] for r in tr) / max(1, len(tr)),
               gnorm_last=tr[-1]["gnorm"] if tr else None, f_last=tr[-1]["f"] if tr else None)
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--memory", type=int, default=5)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--gnorm", type=float, default=1e-6)
    ap.add_argument("--objectives", nargs="*", default=["chain", "lse"])
    a = ap.parse_args()
    import __graft_entry__ as ge
    qn = ge.load_package()
    for lg in a.sizes:
        n = 1 << lg
        rng = np.random.default_rng(5)
        for objective in a.objectives:
            if objective == "chain":
                from test_gpu_device_closure import _Chain
                x0 = rng.uniform(-2.0, 2.0, n)
                ch = _Chain(qn, rng.uniform(0.5, 2.0, n), 0.3)
                oracle, closer = ch.closure, ch.close
            else:
                x0 = rng.standard_normal(n) / np.sqrt(n)
                oracle, closer = qn.LogSumExp(rng.standard_normal((64, n)), rng.standard_normal(64), 0.5), (lambda: None)
            line = dict(n=n, objective=objective, m=a.memory, gnorm=a.gnorm)
            for name, ls in (("wolfe", qn.StrongWolfe(1e-4, 0.9)), ("backtracking", qn.BackTracking(1e-4, 0.5))):
                _run(qn, x0, a.memory, a.gnorm, ls, oracle, 3)  # warm-up: allocations, code objects
                line.update({f"{name}_{k}": v for k, v in _run(qn, x0, a.memory, a.gnorm, ls, oracle, a.iters).items()})
            print(json.dumps(line), flush=True)
            closer()


if __name__ == "__main__":
    main()
