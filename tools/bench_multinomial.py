"""The device multinomial objective (qn.Multinomial, csrc/qn_multinomial.hip.h) beside the logistic objective on a matrix OF THE SAME BYTE
COUNT (the same m, the same n, so the same 8 m n_pad bytes of A), at (m, n, K) = (65536, 784, 10), (65536, 1024, 16), (32768, 2048, 8),
(262144, 256, 64).  Not run by any test.  One JSON line per shape with
  * from profiled qn_minimize calls (NewtonCG + BackTracking, a few iterations, REPS repetitions each; the calls of the objectives INTERLEAVED in one
    process, one objective per call): milliseconds per launch of mnl_onepass_kernel in evaluation mode (t_eval_ms / n_eval_timed: the class brackets the stream of A alone, the combine counts under t_ctl_ms) and
    in product mode (t_newton_ms / n_newton_timed, the figure tools/bench_logistic.py reports for the product's stream), and its
    rate on the byte model 8 m n_pad + 8 m K + 8 G N_pad; beside it logit_onepass_kernel's bracket on its 8 m n_pad bytes, and the ratio of the two
    rates, and the same two brackets with mnl_mfma_kernel streaming A (`set_kernel(2)`, where it is built).  Each minus the fixed part of an event
    bracket;
  * one evaluation from the host (`obj(x)`: the upload of x, two launches, the download of g), median of 10;
  * NewtonCG + BackTracking and LBFGS(5) + StrongWolfe per iteration on the device objective, beside a numpy host closure of the same function.
usage: bench_multinomial.py [m,n,K ...]"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

qn = ge.load_package()

ITERS = 3
LBFGS_ITERS = 5
REPS = 3
shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if not a.startswith("--")] or [(65536, 784, 10), (65536, 1024, 16), (32768, 2048, 8),
                                                                                                   (262144, 256, 64)]


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
    out = dict(eval_ms=st["t_eval_ms"] / max(st["n_eval_timed"], 1) - over, hv_bracket_ms=st["t_newton_ms"] / max(st["n_newton_timed"], 1) - over,
               weights_ms=st["t_ereduce_ms"] / max(st["n_ereduce_timed"], 1) - over, inner_total=s.inner_iterations()[1], iterations=s.k())
    s.close()
    return out


def host_multinomial(a, y, k, mu):
    """the same function as a host closure, in the device's association"""
    m, n = a.shape
    rows = np.arange(m)

    def fn(x):
        wm = x.reshape(k, n)
        z = a @ wm.T
        zmax = z.max(axis=1)
        e = np.exp(z - zmax[:, None])
        s = e.sum(axis=1)
        c = e / s[:, None]
        f = float(np.sum((zmax - z[rows, y]) + np.log(s))) + 0.5 * mu * float(x @ x)
        c[rows, y] = -((s - e[rows, y]) / s)
        return f, (c.T @ a + mu * wm).ravel()
    return fn


for (m, n, k) in shapes:
    rng = np.random.default_rng(3)
    a = rng.standard_normal((m, n))
    y = np.argmax(a @ rng.standard_normal((k, n)).T + 0.5 * rng.gumbel(size=(m, k)), axis=1)
    x0 = 0.01 * rng.standard_normal(k * n)
    xl = 0.01 * rng.standard_normal(n)
    v = rng.standard_normal(k * n)
    mnl, logit = qn.Multinomial(a, y, k, 0.5), qn.Logistic(a, np.where(y > 0, 1.0, -1.0), 0.5)
    mnl.hess_vec_at(x0, v, download=False)  # warm-up: code objects, the LDS attribute
    mnl(x0)
    logit(xl)
    n_pad, nn_pad, g_wg = 16 * ((n + 15) // 16), 16 * ((k * n + 15) // 16), min(256, (16 * ((m + 15) // 16) + 3) // 4)
    model = 8 * m * n_pad + 8 * m * k + 8 * g_wg * nn_pad
    out = dict(m=m, n=n, K=k, library=qn._abi.LIB_PATH, model_bytes=model, a_bytes=8 * m * n_pad)
    bt = qn.BackTracking(1e-4, 0.5)
    run(lambda: qn.NewtonCG(1e-12, x0), bt, mnl, ITERS)[0].close()
    run(lambda: qn.NewtonCG(1e-12, xl), bt, logit, ITERS)[0].close()
    over = qn.default_context().event_bracket_overhead_ms()
    reps = dict(multinomial=[], logistic=[])
    try:
        mnl.set_kernel(2)
        mnl.hess_vec_at(x0, v, download=False)  # (warm-up of the second kernel)
        reps["multinomial_mfma"] = []
    except qn.ErrorInputParams:
        pass
    for _ in range(REPS):  # interleaved: the objectives see the same state of the machine
        mnl.set_kernel(1)
        reps["multinomial"].append(profiled(mnl, x0, over))
        reps["logistic"].append(profiled(logit, xl, over))
        if "multinomial_mfma" in reps:
            mnl.set_kernel(2)
            reps["multinomial_mfma"].append(profiled(mnl, x0, over))
    mnl.set_kernel(0)
    prof = dict(bracket_overhead_ms=round(over, 5))
    for name, rows in reps.items():
        ev = float(np.median([r["eval_ms"] for r in rows]))
        nbytes = 8 * m * n_pad if name == "logistic" else model
        prof[name] = dict(eval_ms=[round(r["eval_ms"], 4) for r in rows], eval_ms_median=round(ev, 4), eval_tb_s=round(nbytes / (ev * 1e-3) / 1e12, 3),
                          a_tb_s=round(8 * m * n_pad / (ev * 1e-3) / 1e12, 3),
                          hv_bracket_ms_median=round(float(np.median([r["hv_bracket_ms"] for r in rows])), 4),
                          weights_ms_median=round(float(np.median([r["weights_ms"] for r in rows])), 4), inner_total=rows[0]["inner_total"],
                          iterations=rows[0]["iterations"])
    prof["a_rate_ratio_multinomial_over_logistic"] = round(prof["multinomial"]["a_tb_s"] / prof["logistic"]["a_tb_s"], 3)
    if "multinomial_mfma" in prof:
        prof["eval_ms_mfma_over_vector"] = round(prof["multinomial_mfma"]["eval_ms_median"] / prof["multinomial"]["eval_ms_median"], 3)
        prof["hv_ms_mfma_over_vector"] = round(prof["multinomial_mfma"]["hv_bracket_ms_median"] / prof["multinomial"]["hv_bracket_ms_median"], 3)
    out["profiled"] = prof
    times = []
    for _ in range(10):
        t0 = time.perf_counter()
        mnl(x0)
        times.append((time.perf_counter() - t0) * 1e3)
    out["eval_call_ms_median"] = round(float(np.median(times)), 4)
    fn = host_multinomial(a, y, k, 0.5)
    for tag, make, ls, iters in (("newton_cg_bt", lambda: qn.NewtonCG(1e-12, x0), bt, ITERS),
                                 ("lbfgs5_wolfe", lambda: qn.LBFGS(1e-12, x0, m=5, memoize=1), qn.StrongWolfe(), LBFGS_ITERS)):
        for name, oracle, reps_n in (("device", mnl, REPS), ("host_closure", fn, 1)):
            if tag == "newton_cg_bt" and name == "host_closure":
                continue  # (a closure has no Hessian-vector product)
            per_iter = []
            for rep in range(reps_n + 1):  # (the first is the warm-up)
                s, ms = run(make, ls, oracle, iters)
                if rep:
                    per_iter.append(ms / max(s.k(), 1))
                s.close()
            out[f"{tag}_{name}_ms_per_iter"] = [round(t, 3) for t in per_iter]
    print(json.dumps(out), flush=True)
    mnl.close()
    logit.close()
