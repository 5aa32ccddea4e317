"""PnormDescent + More-Thuente on Quadratic.synthetic with inverse_p = diag(1 / Q_ii), n = 4096 and 16384.  On this path the
objective is evaluated by quad_matvec_kernel -- the existing mat-vec, one read-only stream of the n x n matrix Q per evaluation -- and the direction
by pnorm_dir_kernel, one read-only stream of inverse_p: the SAME number of bytes per launch, in the same run.  Reported per size:
  * wall time of `minimize` between two context synchronisations, per iteration: five sub-samples (median, min, max);
  * from a profiling run (HIP events around every launch): the direction kernel's time per launch (qn_stats.t_hpass_ms / n_hpass_timed) and
    quad_matvec_kernel's (t_eval_ms / n_eval_timed), bytes per launch, TB/s of each, for every instance of the direction kernel (rows per wave 2 / 4,
    plain / non-temporal loads) -- the non-temporal decision at each size is read off these rows.
usage: bench_pnorm.py [n ...] [--profile]   (--profile: warm runs with the default instance only, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

qn = ge.load_package()
import problems as P  # noqa: E402

ITERS = 12
args = [a for a in sys.argv[1:] if not a.startswith("--")]
sizes = [int(a) for a in args] or [4096, 16384]
profile_only = "--profile" in sys.argv


def timed(x0, p, obj, profiling=False, rw=0, nt=-1):
    s = qn.PnormDescent(1e-12, x0, p)
    s.set_option("pnorm_rows_per_wave", rw)
    s.set_option("pnorm_nontemporal", nt)
    s.set_profiling(profiling)
    qn.default_context().synchronize()
    t0 = time.perf_counter()
    try:
        s.minimize(qn.MoreThuente(), obj, ITERS, 20)
    except qn.MaxIterReached:
        pass
    qn.default_context().synchronize()
    dt = time.perf_counter() - t0
    st, k = s.stats(), s.k()
    s.close()
    return dt * 1e3 / max(k, 1), k, st


def kernel_figures(st, n_pad):
    nbytes = n_pad * n_pad * 8
    d_us = 1e3 * st["t_hpass_ms"] / max(st["n_hpass_timed"], 1)
    q_us = 1e3 * st["t_eval_ms"] / max(st["n_eval_timed"], 1)
    return dict(pnorm_dir_us=round(d_us, 2), pnorm_dir_tb_s=round(nbytes / d_us / 1e6, 3) if d_us else None, launches=st["n_hpass_timed"],
                quad_matvec_us=round(q_us, 2), quad_matvec_tb_s=round(nbytes / q_us / 1e6, 3) if q_us else None, evals=st["n_eval_timed"],
                bytes_per_launch=nbytes, path=st["path"])


for n in sizes:
    diag = P.synth_diag(n, 1e2)
    b, x0 = P.synth_vectors(n)
    obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
    p = np.diag(1.0 / diag)  # Q_ii = diag_i
    n_pad = (n + 15) // 16 * 16
    timed(x0, p, obj)  # warm-up: allocations, code objects
    if profile_only:
        print(f"n={n} profile: k={timed(x0, p, obj)[1]}")
        continue
    ms = [timed(x0, p, obj)[0] for _ in range(5)]
    out = dict(n=n, iters=ITERS, ms_per_iter=[round(v, 4) for v in ms], median=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4))
    for rw in (2, 4):
        for nt in (0, 1):
            out[f"rw{rw}_nt{nt}"] = kernel_figures(timed(x0, p, obj, True, rw, nt)[2], n_pad)
    out["default"] = kernel_figures(timed(x0, p, obj, True)[2], n_pad)
    print(json.dumps(out))
