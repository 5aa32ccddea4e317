"""Broyden + More-Thuente on Quadratic.synthetic beside BFGS on the GENERIC path (QN_OPT_GENERIC_KERNELS 1, QN_OPT_SYMMETRIC_STORAGE 0: full rows of H,
the same 16 n^2 algorithmic bytes per iteration), in one process, alternating (tools/bench_pnewton.py's protocol):
  * wall time of `minimize` between two context synchronisations, per iteration, five alternating repetitions each (median, min-max);
  * the H-pass kernels' own time from a profiling run (HIP events around every launch: qn_stats.t_hpass_ms / n_hpass_timed, the second stage in
    t_hreduce_ms), the bytes qn_stats.h_bytes says those passes moved, bytes/s and the share of the 8 TB/s HBM roofline.
usage: bench_broyden.py [n ...] [--profile]   (--profile: only warm runs of both solvers, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

qn = ge.load_package()
import problems as P  # noqa: E402

ITERS = 6  # (the update as the reference writes it need not keep H positive definite: short calls, as the parity windows)
ROOFLINE = 8.0e12
args = [a for a in sys.argv[1:] if not a.startswith("--")]
sizes = [int(a) for a in args] or [4096, 8192]
profile_only = "--profile" in sys.argv


def make_broyden(x0):
    return qn.Broyden(1e-12, x0)


def make_bfgs_generic(x0):
    s = qn.BFGS(1e-12, x0)
    s.set_option("generic_kernels", 1)
    s.set_option("symmetric_storage", 0)
    s.set_sync_mode(1)  # synchronous requests, as Broyden always runs
    return s


def run(s, obj):
    try:
        s.minimize(qn.MoreThuente(), obj, ITERS, 20)
    except qn.MaxIterReached:
        pass


def timed(make, x0, obj, profiling=False):
    s = make(x0)
    s.set_profiling(profiling)
    qn.default_context().synchronize()
    t0 = time.perf_counter()
    run(s, obj)
    qn.default_context().synchronize()
    dt = time.perf_counter() - t0
    st, k = s.stats(), s.k()
    s.close()
    return dt * 1e3 / max(k, 1), k, st


def pass_figures(st):
    t = st["t_hpass_ms"] * 1e-3
    return dict(h_passes=st["h_passes"], timed=st["n_hpass_timed"], pass_us=round(1e6 * t / max(st["n_hpass_timed"], 1), 2),
                reduce_us=round(1e3 * st["t_hreduce_ms"] / max(st["n_hreduce_timed"], 1), 2), h_bytes=st["h_bytes"],
                tb_per_s=round(st["h_bytes"] / t / 1e12, 3) if t > 0 else None,
                roofline_share=round(st["h_bytes"] / t / ROOFLINE, 3) if t > 0 else None, path=st["path"])


for n in sizes:
    diag = P.synth_diag(n, 1e2)
    b, x0 = P.synth_vectors(n)
    obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
    timed(make_broyden, x0, obj)  # warm-up: allocations, code objects
    timed(make_bfgs_generic, x0, obj)
    if profile_only:
        print(f"n={n} profile: broyden k={timed(make_broyden, x0, obj)[1]} bfgs_generic k={timed(make_bfgs_generic, x0, obj)[1]}")
        continue
    br, bf = [], []
    for rep in range(5):
        bf.append(timed(make_bfgs_generic, x0, obj)[0])
        br.append(timed(make_broyden, x0, obj)[0])
    out = dict(n=n, iters=ITERS, broyden_ms_per_iter=[round(v, 4) for v in br], bfgs_generic_ms_per_iter=[round(v, 4) for v in bf],
               broyden_median=round(float(np.median(br)), 4), bfgs_generic_median=round(float(np.median(bf)), 4),
               broyden_pass=pass_figures(timed(make_broyden, x0, obj, True)[2]),
               bfgs_generic_pass=pass_figures(timed(make_bfgs_generic, x0, obj, True)[2]))
    print(json.dumps(out))
