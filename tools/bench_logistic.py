"""The device logistic objective (qn.Logistic, csrc/qn_logistic.hip.h) beside the log-sum-exp objective ON THE SAME A, m = n = 4096, 8192,
16384.  Not run by any test.  One JSON line per size with
  * from profiled qn_minimize calls (NewtonCG + BackTracking, a few iterations, REPS repetitions each, interleaved): milliseconds per launch of
    logit_onepass_kernel (t_eval_ms / n_eval_timed: for this objective the class brackets the stream of A alone, the combine counts under t_ctl_ms)
    and the bytes/s of 8 m n bytes over it; beside it the log-sum-exp evaluation's bracket (lse_onepass_kernel with its two small launches inside:
    lse_combine_kernel and lse_finish1_kernel) -- the yardstick, with its own spread over the repetitions; the product's stream (t_newton_ms /
    n_newton_timed) and the weights pass (t_ereduce_ms / n_ereduce_timed: one stream and one combine here, four launches and two passes of A for
    log-sum-exp).  Each minus the fixed part of an event bracket.  THE TWO EVALUATION FIGURES ARE NOT THE SAME THING -- one kernel on this side, a
    bracket of three launches on the other -- so no ratio of them is reported: lse_onepass_kernel alone was 7-8 % below its bracket at 8192 / 16384
    (DESIGN.md 26).  Like against like in this call: the whole evaluation from the host, below.  Kernel against kernel, in a run of its own:
        rocprofv3 --kernel-trace --stats -- python tools/bench_logistic.py 16384 --profile
  * one evaluation from the host (`obj(x)`: the upload of x, the launches -- two here, three for log-sum-exp --, the download of g), median of 10;
  * one NewtonCG + BackTracking iteration (wall time of `minimize` per outer iteration, with the inner steps it took) on both objectives;
  * LBFGS(5) + StrongWolfe iterations on the device objective beside a host closure of the same function (numpy, two n-vectors over the bus per
    evaluation).
usage: bench_logistic.py [n ...] [--profile]"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

qn = ge.load_package()

ITERS = 3
LBFGS_ITERS = 5
REPS = 4
args = [a for a in sys.argv[1:] if not a.startswith("--")]
sizes = [int(a) for a in args] or [4096, 8192, 16384]
profile_only = "--profile" in sys.argv


def run(make, ls, oracle, iters):
    s = make()
    qn.default_context().synchronize()
    t0 = time.perf_counter()
    try:
        s.minimize(ls, oracle, iters, 20)
    except qn.MaxIterReached:
        pass
    qn.default_context().synchronize()
    return s, (time.perf_counter() - t0) * 1e3


def profiled(obj, x0, over):
    s = qn.NewtonCG(1e-12, x0)
    s.set_profiling(1)
    try:
        s.minimize(qn.BackTracking(1e-4, 0.5), obj, ITERS, 20)
    except qn.MaxIterReached:
        pass
    st = s.stats()
    out = dict(eval_ms=st["t_eval_ms"] / max(st["n_eval_timed"], 1) - over, hv_ms=st["t_newton_ms"] / max(st["n_newton_timed"], 1) - over,
               weights_ms=st["t_ereduce_ms"] / max(st["n_ereduce_timed"], 1) - over, evals_timed=st["n_eval_timed"], inner_total=s.inner_iterations()[1],
               iterations=s.k())
    s.close()
    return out


def host_logistic(a, yw, mu):
    """the same function as a host closure, in the device's association"""
    at = np.ascontiguousarray(a.T)
    aw = np.abs(yw)

    def fn(x):
        z = np.where(yw < 0.0, -1.0, 1.0) * (a @ x)
        e = np.exp(-np.abs(z))
        q = 1.0 + e
        s = np.where(z >= 0.0, e, 1.0) / q
        f = float(np.sum(aw * (np.maximum(-z, 0.0) + np.log1p(e)))) + 0.5 * mu * float(x @ x)
        return f, at @ (-(yw * s)) + mu * x
    return fn


for n in sizes:
    m = n
    rng = np.random.default_rng(3)
    a, c = rng.standard_normal((m, n)), rng.standard_normal(m)
    xs = rng.standard_normal(n) / np.sqrt(n)
    y = np.where(a @ xs + 0.5 * rng.standard_normal(m) >= 0.0, 1.0, -1.0)
    x0 = 0.01 * rng.standard_normal(n)
    v = rng.standard_normal(n)
    logit, lse = qn.Logistic(a, y, 0.5), qn.LogSumExp(a, c, 0.5)
    for obj in (logit, lse):  # warm-up: code objects, the LDS attribute
        obj.hess_vec_at(x0, v, download=False)
        obj(x0)
    if profile_only:
        for _ in range(4):
            for obj in (logit, lse):
                obj.hess_vec_at(x0, v, download=False)
                obj(x0)
        print(f"n={n} profile: 4 x (hess_vec_at, evaluation) on Logistic and on LogSumExp")
        logit.close()
        lse.close()
        continue
    out = dict(m=m, n=n, library=qn._abi.LIB_PATH, bytes_per_pass=8 * m * n)
    bt = qn.BackTracking(1e-4, 0.5)
    for obj in (logit, lse):
        run(lambda: qn.NewtonCG(1e-12, x0), bt, obj, ITERS)[0].close()  # warm-up
    over = qn.default_context().event_bracket_overhead_ms()
    reps = dict(logistic=[], lse=[])
    for _ in range(REPS):  # interleaved: both objectives see the same state of the machine
        reps["logistic"].append(profiled(logit, x0, over))
        reps["lse"].append(profiled(lse, x0, over))
    prof = dict(bracket_overhead_ms=round(over, 5))
    for name, rows in reps.items():
        ev = [r["eval_ms"] for r in rows]
        what = "stream_kernel_alone" if name == "logistic" else "bracket_of_three_launches"
        prof[name] = dict(eval_bracket_holds=what, eval_ms=[round(t, 4) for t in ev], eval_ms_median=round(float(np.median(ev)), 4),
                          eval_ms_spread=round(max(ev) - min(ev), 4), eval_tb_s=round(8 * m * n / (float(np.median(ev)) * 1e-3) / 1e12, 3),
                          hv_ms_median=round(float(np.median([r["hv_ms"] for r in rows])), 4),
                          weights_ms_median=round(float(np.median([r["weights_ms"] for r in rows])), 4),
                          evals_timed=rows[0]["evals_timed"], inner_total=rows[0]["inner_total"], iterations=rows[0]["iterations"])
    out["profiled"] = prof
    for name, obj in (("logistic", logit), ("lse", lse)):
        times = []
        for _ in range(10):
            t0 = time.perf_counter()
            obj(x0)
            times.append((time.perf_counter() - t0) * 1e3)
        out[f"{name}_eval_call_ms_median"] = round(float(np.median(times)), 4)
        per_iter, inner = [], []
        for rep in range(REPS):
            s, ms = run(lambda: qn.NewtonCG(1e-12, x0), bt, obj, ITERS)
            per_iter.append(ms / max(s.k(), 1))
            inner.append(s.inner_iterations()[1] / max(s.k(), 1))
            s.close()
        out[f"{name}_newton_cg_bt_ms_per_iter"] = [round(t, 3) for t in per_iter]
        out[f"{name}_newton_cg_bt_median"] = round(float(np.median(per_iter)), 3)
        out[f"{name}_inner_steps_per_iter"] = round(float(np.median(inner)), 2)
    fn = host_logistic(a, y, 0.5)
    for name, oracle, reps_n in (("device", logit, REPS), ("host_closure", fn, 2)):
        per_iter = []
        for rep in range(reps_n + 1):  # (the first is the warm-up)
            s, ms = run(lambda: qn.LBFGS(1e-12, x0, m=5, memoize=1), qn.StrongWolfe(), oracle, LBFGS_ITERS)
            if rep:
                per_iter.append(ms / max(s.k(), 1))
            evals = s.stats()["oracle_evals"]
            s.close()
        out[f"lbfgs5_wolfe_{name}_ms_per_iter"] = [round(t, 3) for t in per_iter]
        out[f"lbfgs5_wolfe_{name}_median"] = round(float(np.median(per_iter)), 3)
        out[f"lbfgs5_wolfe_{name}_evals"] = int(evals)
    print(json.dumps(out), flush=True)
    logit.close()
    lse.close()
