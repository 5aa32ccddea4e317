"""Measurements of OWLQN.  A tool, not a test.

  kernels   owl_pg_kernel, owl_dir_kernel and owl_trial_kernel beside prox_dir_kernel and prox_trial_kernel, and owl_accept_kernel beside
            lbfgs_accept_kernel, at n = 2^20, 2^22, 2^24: one child process under `rocprofv3 --kernel-trace` runs LBFGS, SpectralProximalGradient and
            OWLQN (scalar and vector l1) on the same device closure (examples/device_closure.hip) at every size, a prim_axpy_kernel launch marking
            each size's start; the trace is read here, the median duration of every kernel per size is set against the bytes of its model:
                owl_pg_kernel<L1VEC>           16 n (x, g) + 8 n if L1VEC read, 8 n written (v)
                owl_dir_kernel<L1VEC>          16 n (z, v) + 8 n if L1VEC read, 8 n written (d)
                owl_trial_kernel<L1VEC>        24 n (x, d, v) + 8 n if L1VEC read, 8 n written (xt)
                owl_accept_kernel              32 n (x, xt, g, gt) read, 32 n written (s, y, g, x)
                lbfgs_accept_kernel            32 n (x, d, g, gt) read, 32 n written
                prox_dir_kernel<false, L1VEC>  16 n + 8 n if L1VEC read, 8 n written;  prox_trial_kernel<L1VEC>  16 n + 8 n if L1VEC read, 8 n written
  runs      whole runs to a common tolerance: OWLQN(m = 5) + BackTracking(1e-4, 0.5) beside SpectralProximalGradient + GLLQuadratic(1e-4, 10), the
            settings alternating in one session, on L1 SparseLogistic at m = n = 2^20 with 16 nonzeros per row and on the dense Logistic at
            8192 x 8192; wall time, iterations, oracle evaluations and nonzeros of each.

    python tools/bench_owlqn.py [kernels] [runs] [--sizes 1048576,4194304,16777216] [--iters 20] [--tol 1e-4] [--cap 400] [--out build/owlqn_prof]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_prox import MARKER, _flags  # noqa: E402


def model_bytes(name, n):
    if "owl_pg_kernel" in name or "owl_dir_kernel" in name:
        return (24 + (8 if _flags(name)[0] else 0)) * n
    if "owl_trial_kernel" in name:
        return (32 + (8 if _flags(name)[0] else 0)) * n
    if "owl_accept_kernel" in name or "lbfgs_accept_kernel" in name:
        return 64 * n
    if "prox_dir_kernel" in name:
        boxed, vec = _flags(name)
        return (24 + (16 if boxed else 0) + (8 if vec else 0)) * n
    if "prox_trial_kernel" in name:
        return (24 + (8 if _flags(name)[0] else 0)) * n
    return None


def child(sizes, iters):
    """every variant at every size, in one process; run under rocprofv3 by `kernels`"""
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)
    import __graft_entry__ as ge
    from tools.bench_spg import Chain
    qn = ge.load_package()
    ctx = qn.default_context()
    tiny = qn.DeviceBuffer(ctx, np.zeros(2))
    for n in sizes:
        qn.axpy(ctx, 2, tiny, 0.0, tiny, tiny)  # the marker in front of this size's launches
        rng = np.random.default_rng(5)
        av, x0 = rng.uniform(0.5, 2.0, n), rng.uniform(-2.0, 2.0, n)
        ch = Chain(qn, av, 0.3)
        l1v = np.full(n, 0.05)
        # memoize = 1: the accepted trial's evaluation is kept, so every trial-kernel launch that works is in phase QN_VP_TRIAL (the model's bytes)
        runs = [(lambda: qn.LBFGS(1e-12, x0, memoize=1), qn.BackTracking(1e-4, 0.5))]
        for vec in (False, True):
            runs.append((lambda vec=vec: qn.SpectralProximalGradient(1e-12, x0, ch.closure, l1v if vec else 0.05, memoize=1), qn.GLLQuadratic(1e-4, 10)))
            runs.append((lambda vec=vec: qn.OWLQN(1e-12, x0, l1v if vec else 0.05, memoize=1), qn.BackTracking(1e-4, 0.5)))
        for make, ls in runs:
            s = make()
            try:
                s.minimize(ls, ch.closure, iters, 50)
            except qn.MaxIterReached:
                pass
            s.close()
        ch.close()


def kernels(sizes, iters, out):
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--child",
           "--sizes", ",".join(str(n) for n in sizes), "--iters", str(iters)]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=900, stdout=subprocess.DEVNULL)
    f = glob.glob(os.path.join(out, "**", "p_kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    seg = -1
    dur = {}
    for r in rows:
        name = r["Kernel_Name"]
        if MARKER in name:
            seg += 1
            continue
        if seg < 0 or seg >= len(sizes) or model_bytes(name, 1) is None:
            continue
        dur.setdefault((seg, name.split("(")[0].replace("void ", "")), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (seg, name), us in sorted(dur.items()):
        n = sizes[seg]
        # launches predicated off return in a few microseconds (the phase did not match): the median of the launches that did the work
        work = [u for u in us if u > 0.5 * max(us)]
        med = statistics.median(work)
        print(json.dumps(dict(what="kernel", n=n, kernel=name, launches=len(us), timed=len(work), us_median=round(med, 2), us_min=round(min(work), 2),
                              model_bytes=model_bytes(name, n), gb_per_s=round(model_bytes(name, n) / med / 1e3, 1))), flush=True)


def _sparse_logistic(qn):
    m = n = 1 << 20
    per_row = 16
    rng = np.random.default_rng(7)
    block = n // per_row  # one column from each sixteenth of the range: sorted and distinct inside a row
    cols = np.arange(per_row, dtype=np.int64)[None, :] * block + rng.integers(0, block, size=(m, per_row), dtype=np.int64)
    indptr = np.arange(0, m * per_row + 1, per_row, dtype=np.int64)
    data = rng.standard_normal(m * per_row) / 4.0
    xs = np.where(rng.random(n) < 0.01, rng.standard_normal(n), 0.0)
    margins = np.add.reduceat(data * xs[cols.ravel()], indptr[:-1])
    y = np.where(margins + 0.1 * rng.standard_normal(m) >= 0.0, 1.0, -1.0)
    return qn.SparseLogistic(indptr, cols.ravel(), data, y, 1e-3, n), n


def _dense_logistic(qn):
    m = n = 8192
    rng = np.random.default_rng(9)
    a = rng.standard_normal((m, n)) / np.sqrt(n)
    xs = np.where(rng.random(n) < 0.03, 4.0 * rng.standard_normal(n), 0.0)
    y = np.where(a @ xs + 0.1 * rng.standard_normal(m) >= 0.0, 1.0, -1.0)
    return qn.Logistic(a, y, 1e-3), n


def runs(tol, cap, l1s):
    import torch  # noqa: F401
    import __graft_entry__ as ge
    qn = ge.load_package()
    for name, make_obj in (("sparse_logistic_2^20", _sparse_logistic), ("logistic_8192", _dense_logistic)):
        obj, n = make_obj(qn)
        x0 = np.zeros(n)
        l1 = l1s[name]
        out = {"owlqn": [], "prox": []}
        for rep in range(4):  # the settings alternate; the first pair warms up
            for which in ("owlqn", "prox"):
                s = qn.OWLQN(tol, x0, l1) if which == "owlqn" else qn.SpectralProximalGradient(tol, x0, obj, l1)
                ls = qn.BackTracking(1e-4, 0.5) if which == "owlqn" else qn.GLLQuadratic(1e-4, 10)
                t0 = time.perf_counter()
                try:
                    s.minimize(ls, obj, cap, 50)
                    status = "ok"
                except qn.MaxIterReached:
                    status = "max_iter"
                dt = time.perf_counter() - t0  # (qn_minimize returns behind its last synchronisation)
                st = s.stats()
                rec = dict(ms=round(1e3 * dt, 2), status=status, iterations=int(st["iterations"]), evals=int(st["oracle_evals"]), nonzeros=int(np.count_nonzero(s.x())))
                s.close()
                if rep:
                    out[which].append(rec)
        obj.close()
        summary = {}
        for which, recs in out.items():
            ms = sorted(r["ms"] for r in recs)
            summary[which] = dict(ms_min=ms[0], ms_median=ms[len(ms) // 2], ms_max=ms[-1], **{k: recs[-1][k] for k in ("status", "iterations", "evals", "nonzeros")})
        print(json.dumps(dict(what="whole_runs", problem=name, n=n, l1=l1, tol=tol, cap=cap, **summary)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "runs"])
    ap.add_argument("--sizes", default="1048576,4194304,16777216")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--cap", type=int, default=400)
    ap.add_argument("--l1-sparse", type=float, default=1.0)
    ap.add_argument("--l1-dense", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "owlqn_prof"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    if a.child:
        return child(sizes, a.iters)
    if "kernels" in a.what:
        kernels(sizes, a.iters, os.path.abspath(a.out))  # (the child runs from the tree's root)
    if "runs" in a.what:
        runs(a.tol, a.cap, {"sparse_logistic_2^20": a.l1_sparse, "logistic_8192": a.l1_dense})


if __name__ == "__main__":
    main()
