"""Truncated Newton on the device log-sum-exp objective (QN_NEWTON_CG, csrc/qn_newton_cg.hip.h; the product: csrc/qn_lse_hv.hip.h),
m = n = 4096, 8192, 16384.  Not run by any test.  One JSON line per size with
  * from ONE profiled qn_minimize call (NewtonCG + BackTracking, a few iterations) on one matrix A: milliseconds per launch of the product's stream
    of A, lse_hv_onepass_kernel (t_newton_ms / n_newton_timed: the class also brackets lse_hv_combine_kernel, whose launches fall under the
    class's floor of half a long launch and are not averaged in), beside the evaluation (t_eval_ms / n_eval_timed: ONE bracket around
    lse_onepass_kernel, lse_combine_kernel and lse_finish1_kernel -- the two small launches are inside it), each minus the fixed part of an event
    bracket, and the bytes/s of 8 m n bytes over each.  Kernel against kernel, without the evaluation's two small launches: a trace in a run of its own,
        rocprofv3 --kernel-trace --stats -- python tools/bench_newton_cg.py 16384 --profile
  * one NewtonCG + BackTracking iteration (wall time of `minimize` per outer iteration, with the inner steps it took) beside one Newton +
    More-Thuente iteration at the sizes where Newton's n x n matrix is formed (n <= 8192 here: 2 GB at 16384).
usage: bench_newton_cg.py [n ...] [--profile] [--no-newton]"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

qn = ge.load_package()

ITERS = 3
REPS = 4
args = [a for a in sys.argv[1:] if not a.startswith("--")]
sizes = [int(a) for a in args] or [4096, 8192, 16384]
profile_only = "--profile" in sys.argv


def run(make, ls, obj, iters):
    s = make()
    qn.default_context().synchronize()
    t0 = time.perf_counter()
    try:
        s.minimize(ls, obj, iters, 20)
    except qn.MaxIterReached:
        pass
    qn.default_context().synchronize()
    return s, (time.perf_counter() - t0) * 1e3


for n in sizes:
    m = n
    rng = np.random.default_rng(3)
    a, c = rng.standard_normal((m, n)), rng.standard_normal(m)
    x0 = 0.01 * rng.standard_normal(n)  # (every row carries weight; timing does not depend on it)
    obj = qn.LogSumExp(a, c, 0.5)
    del a
    v = rng.standard_normal(n)
    obj.hess_vec_at(x0, v, download=False)  # warm-up: code objects, the LDS attribute
    obj(x0)
    if profile_only:
        for _ in range(4):
            obj.hess_vec_at(x0, v, download=False)
            obj(x0)
        print(f"n={n} profile: 4 x (hess_vec_at, evaluation)")
        obj.close()
        continue
    out = dict(m=m, n=n, library=qn._abi.LIB_PATH, bytes_per_pass=8 * m * n)
    bt = qn.BackTracking(1e-4, 0.5)
    run(lambda: qn.NewtonCG(1e-12, x0), bt, obj, ITERS)[0].close()  # warm-up
    s = qn.NewtonCG(1e-12, x0)
    s.set_profiling(1)
    try:
        s.minimize(bt, obj, ITERS, 20)
    except qn.MaxIterReached:
        pass
    st = s.stats()
    over = qn.default_context().event_bracket_overhead_ms()
    hv_ms = st["t_newton_ms"] / max(st["n_newton_timed"], 1) - over
    ev_ms = st["t_eval_ms"] / max(st["n_eval_timed"], 1) - over
    out["profiled"] = dict(hv_onepass_ms=round(hv_ms, 4), hv_launches_timed=st["n_newton_timed"], eval_chain_ms=round(ev_ms, 4),
                           eval_launches_timed=st["n_eval_timed"], hv_tb_s=round(8 * m * n / (hv_ms * 1e-3) / 1e12, 3),
                           eval_tb_s=round(8 * m * n / (ev_ms * 1e-3) / 1e12, 3), hv_over_eval=round(hv_ms / ev_ms, 4),
                           weights_ms=round(st["t_ereduce_ms"] / max(st["n_ereduce_timed"], 1), 4), bracket_overhead_ms=round(over, 5),
                           inner_total=s.inner_iterations()[1], iterations=s.k())
    s.close()
    per_iter, inner = [], []
    for rep in range(REPS):
        s, ms = run(lambda: qn.NewtonCG(1e-12, x0), bt, obj, ITERS)
        per_iter.append(ms / max(s.k(), 1))
        inner.append(s.inner_iterations()[1] / max(s.k(), 1))
        s.close()
    out["newton_cg_bt_ms_per_iter"] = [round(t, 3) for t in per_iter]
    out["newton_cg_bt_median"] = round(float(np.median(per_iter)), 3)
    out["inner_steps_per_iter"] = round(float(np.median(inner)), 2)
    if n <= 8192 and "--no-newton" not in sys.argv:
        per_iter = []
        for rep in range(REPS):  # (the first is the warm-up: the work matrix, the factorisation's code objects)
            s, ms = run(lambda: qn.Newton(1e-12, x0), qn.MoreThuente(), obj, ITERS)
            if rep:
                per_iter.append(ms / max(s.k(), 1))
            s.close()
        out["newton_mt_ms_per_iter"] = [round(t, 3) for t in per_iter]
        out["newton_mt_median"] = round(float(np.median(per_iter)), 3)
    print(json.dumps(out), flush=True)
    obj.close()
