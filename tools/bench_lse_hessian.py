"""The log-sum-exp Hessian on the device (csrc/qn_lse_hess.hip.h), m = n = 2048, 4096, 8192:
  * the Hessian launch chain alone: Objective.hessian(x, download=False) between two synchronisations -- the upload of x (8 n bytes), five
    launches (z = A x, softmax, column sums, their fold, lse_hess_kernel) and the wait.  One warm-up, then ROUNDS rounds, median / min / max;
    TFLOP/s counting m n^2 multiply-adds on the half (2 flop each: m n^2 flop), as a share of the 78.6 TFLOP/s f64 MFMA peak and beside
    chol_syrk_kernel's bulk rate (45 TFLOP/s, qn_host_newton.hip.h).  The fixed part (copy, launch overheads, the four small kernels) is a
    visible share at n = 2048; lse_hess_kernel's own time comes from a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats -- python tools/bench_lse_hessian.py 8192 --profile
  * one full Newton + More-Thuente iteration on log-sum-exp at the largest size (wall time of `minimize` per iteration).
The library carries the 64 x 64-tile instance of the kernel.  The 128 x 128 one is a diagnostic build, timed by pointing QN_HIP_LIB at it:
    make -C optimization-solvers_amd/csrc XFLAGS=-DQN_LSE_HESS_TILE=128 OUT=../lib/libqn_hip_tile128.so
usage: bench_lse_hessian.py [n ...] [--profile] [--no-newton]"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

qn = ge.load_package()

ROUNDS = 7
NEWTON_ITERS = 3
PEAK, SYRK = 78.6e12, 45.0e12
args = [a for a in sys.argv[1:] if not a.startswith("--")]
sizes = [int(a) for a in args] or [2048, 4096, 8192]
profile_only = "--profile" in sys.argv


def chain_ms(obj, x):
    qn.default_context().synchronize()
    t0 = time.perf_counter()
    obj.hessian(x, download=False)
    return (time.perf_counter() - t0) * 1e3


def figures(ms, m, n):
    med = float(np.median(ms))
    rate = m * n * n / (med * 1e-3)
    return dict(median_ms=round(med, 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), tflops=round(rate / 1e12, 2),
                share_of_peak=round(rate / PEAK, 3), vs_chol_syrk=round(rate / SYRK, 3))


for n in sizes:
    m = n
    rng = np.random.default_rng(3)
    a, c = rng.standard_normal((m, n)), rng.standard_normal(m)
    x0 = 0.01 * rng.standard_normal(n)  # (every row carries weight; timing does not depend on it)
    obj = qn.LogSumExp(a, c, 0.5)
    chain_ms(obj, x0)  # warm-up: allocation of the device matrix, code objects
    if profile_only:
        for _ in range(4):
            chain_ms(obj, x0)
        print(f"n={n} profile: 5 launches")
        obj.close()
        continue
    out = dict(m=m, n=n, rounds=ROUNDS, library=qn._abi.LIB_PATH, chain=figures([chain_ms(obj, x0) for _ in range(ROUNDS)], m, n))
    if n == max(sizes) and "--no-newton" not in sys.argv:
        per_iter = []
        for rep in range(4):  # (the first is the warm-up: the work matrix, the factorisation's code objects)
            s = qn.Newton(1e-12, x0)
            qn.default_context().synchronize()
            t0 = time.perf_counter()
            try:
                s.minimize(qn.MoreThuente(), obj, NEWTON_ITERS, 20)
            except qn.MaxIterReached:
                pass
            qn.default_context().synchronize()
            if rep:
                per_iter.append((time.perf_counter() - t0) * 1e3 / max(s.k(), 1))
            s.close()
        out["newton_mt_ms_per_iter"] = [round(v, 3) for v in per_iter]
        out["newton_mt_median"] = round(float(np.median(per_iter)), 3)
    print(json.dumps(out), flush=True)
    obj.close()
