"""Measurements of the first-order family ("The first-order family"):
  (a) ProjectedGradientDescent (infinite box) + BackTracking on the device-wide vector kernels against GradientDescent + BackTracking on the
      one-workgroup control kernel, the same device closure (examples/device_closure.hip), n = 4096, 2^18, 2^22, 2^24;
  (b) SpectralProjectedGradient + GLLQuadratic(1e-4, 10) on Quadratic.synthetic at n = 4096: iterations/s, evaluations per iteration.
Warm-up call, then five timed sub-samples; min / median / max.      python tools/bench_spg.py [--iters 40] [--sizes 4096,262144]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process)
import __graft_entry__ as ge  # noqa: E402


class Chain:
    """examples/libdevice_closure.so (examples/device_closure.hip, built by build()): the double-well chain as a device closure"""

    def __init__(self, qn, a, c):
        import ctypes as C
        self.dll = C.CDLL(os.path.join(ROOT, "examples", "libdevice_closure.so"))
        self.dll.double_well_chain_create.restype = C.c_void_p
        self.dll.double_well_chain_create.argtypes = [C.c_size_t, C.POINTER(C.c_double), C.c_double]
        self.dll.double_well_chain_destroy.argtypes = [C.c_void_p]
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.user = self.dll.double_well_chain_create(a.size, a.ctypes.data_as(C.POINTER(C.c_double)), float(c))
        self.closure = qn.DeviceClosure(self.dll.double_well_chain_eval, self.user, keep=self)

    def close(self):
        self.dll.double_well_chain_destroy(self.user)


def timed(make, run, iters, samples=5):
    out = []
    for i in range(samples + 1):
        s = make()
        t0 = time.perf_counter()
        done = run(s)
        dt = time.perf_counter() - t0
        st = s.stats()
        s.close()
        if i:  # the first is the warm-up
            out.append((dt / max(done, 1), st))
    ms = sorted(1e3 * o[0] for o in out)
    st = out[-1][1]
    return dict(ms_per_iter_min=ms[0], ms_per_iter_median=ms[len(ms) // 2], ms_per_iter_max=ms[-1], iterations=int(st["iterations"]),
                evals_per_iter=st["oracle_evals"] / max(st["iterations"], 1), host_syncs=int(st["host_syncs"]), path=int(st["path"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--sizes", default="4096,262144,4194304,16777216")
    a = ap.parse_args()
    qn = ge.load_package()
    seed = 0x5EED0001
    for n in [int(v) for v in a.sizes.split(",")]:
        rng = np.random.default_rng(5)
        av, x0 = rng.uniform(0.5, 2.0, n), rng.uniform(-2.0, 2.0, n)
        ch = Chain(qn, av, 0.3)
        inf = np.full(n, np.inf)

        def run(s):
            try:
                s.minimize(qn.BackTracking(1e-4, 0.5), ch.closure, a.iters, 50)
            except qn.MaxIterReached:
                pass
            return s.k()
        new = timed(lambda: qn.ProjectedGradientDescent(1e-12, x0, -inf, inf), run, a.iters)
        old = timed(lambda: qn.GradientDescent(1e-12, x0), run, a.iters)
        ch.close()
        print(json.dumps(dict(what="pgd_vs_gd_device_closure", n=n, vector_kernels=new, control_kernel=old,
                              speedup_median=old["ms_per_iter_median"] / new["ms_per_iter_median"])), flush=True)
    n = 4096
    diag = 1e2 ** (np.arange(n, dtype=np.float64) / (n - 1))  # kappa = 1e2, as tests/problems.py::synth_diag
    rng = np.random.Generator(np.random.Philox(key=seed))
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    obj = qn.Quadratic.synthetic(n, seed, diag, b)
    lb, ub = np.full(n, -0.05), np.full(n, 0.05)

    def run_spg(s):
        try:
            s.minimize(qn.GLLQuadratic(1e-4, 10), obj, 200, 50)
        except qn.MaxIterReached:
            pass
        return s.k()
    r = timed(lambda: qn.SpectralProjectedGradient(1e-12, x0, obj, lb, ub), run_spg, 200)
    r["iterations_per_s_median"] = 1e3 / r["ms_per_iter_median"]
    print(json.dumps(dict(what="spg_gll_quadratic_synthetic", n=n, **r)), flush=True)


if __name__ == "__main__":
    main()
