"""Measurements of SpectralProximalGradient.  A tool, not a test.

  kernels   prox_dir_kernel's four instances beside vec_dir_kernel, and prox_trial_kernel's two beside vec_trial_kernel, at n = 2^20, 2^22, 2^24:
            one child process under `rocprofv3 --kernel-trace` runs SpectralProjectedGradient (boxed) and the four SpectralProximalGradient instances
            on the same device closure (examples/device_closure.hip) at every size, a prim_axpy_kernel launch marking each size's start; the trace is
            read here, the median duration of every kernel per size is set against the bytes of its model:
                vec_dir_kernel                 32 n read (x, g, lb, ub) + 8 n written (d)
                prox_dir_kernel<BOXED, L1VEC>  16 n (x, g) + 16 n if BOXED + 8 n if L1VEC read, 8 n written
                vec_trial_kernel               16 n read (x, d) + 8 n written (xt)
                prox_trial_kernel<L1VEC>       16 n + 8 n if L1VEC read, 8 n written
  iters     whole iterations on SparseLogistic at m = n = 2^20 with 16 nonzeros per row: SpectralProximalGradient (scalar l1, no box) beside
            SpectralProjectedGradient (infinite box) on the same objective, GLLQuadratic(1e-4, 10); warm-up call, then five timed samples.

    python tools/bench_prox.py [kernels] [iters] [--sizes 1048576,4194304,16777216] [--iters 20] [--out build/prox_prof] [--only spg]
(--only spg: SpectralProjectedGradient alone, which a checkout without this method can run too -- its figures beside this one's in one session)"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARKER = "prim_axpy_kernel"


def _flags(name):
    """the bool template arguments of a kernel name, demangled (`<true, false>`) or mangled (`ILb1ELb0EE`)"""
    if "<" in name:
        return [v.strip() in ("true", "1", "(bool)1") for v in name.split("<")[1].split(">")[0].split(",")]
    return [v == "1" for v in re.findall(r"Lb([01])E", name)]


def model_bytes(name, n):
    if "vec_dir_kernel" in name:
        return 40 * n
    if "prox_dir_kernel" in name:
        boxed, vec = _flags(name)
        return (24 + (16 if boxed else 0) + (8 if vec else 0)) * n
    if "vec_trial_kernel" in name:
        return 24 * n
    if "prox_trial_kernel" in name:
        return (24 + (8 if _flags(name)[0] else 0)) * n
    return None


def child(sizes, iters, only):
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
        lb, ub = np.full(n, -1.5), np.full(n, 1.5)
        l1v = np.full(n, 0.05)
        # memoize = 1: the accepted trial's evaluation is kept, so every trial-kernel launch that works is in phase QN_VP_TRIAL (the model's bytes)
        makers = [lambda: qn.SpectralProjectedGradient(1e-12, x0, ch.closure, lb, ub, memoize=1)] if only != "prox" else []
        for boxed in (False, True):
            for vec in (False, True):
                if only != "spg":
                    makers.append(lambda boxed=boxed, vec=vec: qn.SpectralProximalGradient(1e-12, x0, ch.closure, l1v if vec else 0.05,
                                                                                            lb if boxed else None, ub if boxed else None, memoize=1))
        for make in makers:
            s = make()
            try:
                s.minimize(qn.GLLQuadratic(1e-4, 10), ch.closure, iters, 50)
            except qn.MaxIterReached:
                pass
            s.close()
        ch.close()


def kernels(sizes, iters, out, only):
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--child",
           "--sizes", ",".join(str(n) for n in sizes), "--iters", str(iters), "--only", only]
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


def iterations(iters, only):
    import torch  # noqa: F401
    import __graft_entry__ as ge
    qn = ge.load_package()
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
    obj = qn.SparseLogistic(indptr, cols.ravel(), data, y, 1e-3, n)
    x0 = np.zeros(n)
    inf = np.full(n, np.inf)
    out = {}
    for name, make in (("spg", lambda: qn.SpectralProjectedGradient(1e-12, x0, obj, -inf, inf)),
                       ("prox", lambda: qn.SpectralProximalGradient(1e-12, x0, obj, 0.05))):
        if only not in ("both", name):
            continue
        samples = []
        for i in range(6):
            s = make()
            t0 = time.perf_counter()
            try:
                s.minimize(qn.GLLQuadratic(1e-4, 10), obj, iters, 50)
            except qn.MaxIterReached:
                pass
            dt = time.perf_counter() - t0  # (qn_minimize returns behind its last synchronisation)
            st = s.stats()
            nz = int(np.count_nonzero(s.x()))
            s.close()
            if i:
                samples.append(1e3 * dt / max(st["iterations"], 1))
        samples.sort()
        out[name] = dict(ms_per_iter_min=samples[0], ms_per_iter_median=samples[len(samples) // 2], ms_per_iter_max=samples[-1],
                         iterations=int(st["iterations"]), evals_per_iter=st["oracle_evals"] / max(st["iterations"], 1), nonzeros=nz)
    obj.close()
    if only == "both":
        out["prox_over_spg_median"] = out["prox"]["ms_per_iter_median"] / out["spg"]["ms_per_iter_median"]
    print(json.dumps(dict(what="sparse_logistic_iterations", m=m, n=n, nnz_per_row=per_row, l1=0.05, **out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "iters"])
    ap.add_argument("--sizes", default="1048576,4194304,16777216")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "prox_prof"))
    ap.add_argument("--only", default="both", choices=["both", "spg", "prox"])  # spg: what a library without the method can run
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    if a.child:
        return child(sizes, a.iters, a.only)
    if "kernels" in a.what:
        kernels(sizes, a.iters, os.path.abspath(a.out), a.only)  # (the child runs from the tree's root)
    if "iters" in a.what:
        iterations(a.iters, a.only)


if __name__ == "__main__":
    main()
