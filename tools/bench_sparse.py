"""Measures the sparse quadratic objective (qn.SparseQuadratic, csrc/qn_sparse.hip.h).  Not run by any test.

Shapes: the 2-D five-point Laplacian plus a shift of 0.05 at n = 2^20, 2^22 and 2^24 (banded: x is reused from L2), and a uniformly random symmetric
pattern of about 16 entries per row at n = 2^22 (x gathered from all over the Infinity Cache / HBM).  Per shape, one JSON line per
lanes_per_row with
  * spq_eval_kernel's time per launch: profiling mode brackets it on its own (t_eval_ms; the one-workgroup finish counts under t_ctl_ms), minus the
    fixed part of an event bracket (Context.event_bracket_overhead_ms), over the evaluations of one LBFGS(m = 5) + StrongWolfe call that continues
    a warm-up call;
  * model bytes / time in TB/s, model bytes = 12 nnz + 4 (n + 1) + 24 n (values and columns, row offsets, x read, b read, g written);
then one line with the yardstick -- torch's own torch.mv on the same torch.sparse_csr_tensor (int32 indices), which computes Q x only, so its model is
12 nnz + 4 (n + 1) + 16 n and the ratio of the two models is the allowance for forming g and f as well -- and with whole LBFGS(m = 5) + StrongWolfe
iterations (wall clock per iteration of one qn_minimize call) on the device objective and on a host closure of the same function (scipy's CSR product
when scipy is there, numpy.bincount otherwise).  If torch's sparse CSR mv is not available in the build, the line says so and has no yardstick.

    python tools/bench_sparse.py [--shapes lap20 lap22 lap24 rand22] [--lanes 0 1 2 4 8 16 32 64] [--iters 8] [--host-iters 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def laplacian(side, shift=0.05):
    """CSR of the five-point Laplacian on a side x side grid plus shift I, built in row order (no sort): int32 indices"""
    n = side * side
    r = np.arange(n, dtype=np.int64)
    i, j = r // side, r % side
    cols = np.stack([r - side, r - 1, r, r + 1, r + side], axis=1)
    keep = np.stack([i > 0, j > 0, np.ones(n, dtype=bool), j + 1 < side, i + 1 < side], axis=1)
    vals = np.broadcast_to(np.array([-1.0, -1.0, 4.0 + shift, -1.0, -1.0]), (n, 5))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return indptr.astype(np.int32), cols[keep].astype(np.int32), np.ascontiguousarray(vals[keep])


def random_symmetric(n, per_row=16, seed=7):
    """A + A' of a pattern with per_row / 2 uniformly random columns per row, entries -1 / per_row, diagonal = row sum of magnitudes + 0.05"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    half = per_row // 2
    rows = np.repeat(np.arange(n, dtype=np.int64), half)
    cols = rng.integers(0, n, size=n * half, dtype=np.int64)
    off = rows != cols
    a = sp.csr_matrix((np.full(int(off.sum()), -1.0 / per_row), (rows[off], cols[off])), shape=(n, n))
    a = a + a.T  # (duplicates are summed: still symmetric)
    a = a + sp.diags(np.asarray(abs(a).sum(axis=1)).ravel() + 0.05)
    a = a.tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data


SHAPES = {"lap20": lambda: laplacian(1 << 10), "lap22": lambda: laplacian(1 << 11), "lap24": lambda: laplacian(1 << 12),
          "rand22": lambda: random_symmetric(1 << 22)}


def _minimize(qn, s, ls, oracle, iters):
    t0 = time.perf_counter()
    try:
        s.minimize(ls, oracle, iters, 50)
    except qn.MaxIterReached:
        pass
    qn.default_context().synchronize()
    return time.perf_counter() - t0


def kernel_time_us(qn, obj, x0, iters, bracket_ms):
    s = qn.LBFGS(0.0, x0, m=5, memoize=1)
    _minimize(qn, s, qn.StrongWolfe(1e-4, 0.9), obj, 3)
    before = s.stats()
    s.set_profiling(1)
    _minimize(qn, s, qn.StrongWolfe(1e-4, 0.9), obj, iters)
    st = s.stats()
    s.close()
    cnt = st["n_eval_timed"] - before["n_eval_timed"]
    return (1e3 * ((st["t_eval_ms"] - before["t_eval_ms"]) / cnt - bracket_ms), cnt) if cnt else (None, 0)


def torch_mv_us(indptr, cols, vals, x, reps=20):
    import torch
    dev = torch.device("cuda")
    q = torch.sparse_csr_tensor(torch.from_numpy(indptr).to(dev), torch.from_numpy(cols).to(dev), torch.from_numpy(vals).to(dev),
                                size=(x.size, x.size), dtype=torch.float64, device=dev)
    xv = torch.from_numpy(x).to(dev)
    for _ in range(3):
        y = torch.mv(q, xv)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        y = torch.mv(q, xv)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps, y.cpu().numpy()


def host_closure(indptr, cols, vals, b):
    try:
        import scipy.sparse as sp
        q = sp.csr_matrix((vals, cols, indptr), shape=(b.size, b.size))
        mv = q.dot
    except ImportError:
        rows = np.repeat(np.arange(b.size, dtype=np.int64), np.diff(indptr))

        def mv(x):
            return np.bincount(rows, weights=vals * x[cols], minlength=b.size)

    def fn(x):
        qx = mv(x)
        return 0.5 * float(x @ qx) - float(b @ x), qx - b
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--lanes", type=int, nargs="*", default=[0, 1, 2, 4, 8, 16, 32, 64])
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--host-iters", type=int, default=4)
    a = ap.parse_args()
    try:
        import torch  # noqa: F401 -- before libqn_hip.so is loaded, so that one HIP runtime serves both (tests/conftest.py says why)
    except ImportError:
        pass
    import __graft_entry__ as ge
    qn = ge.load_package()
    bracket_ms = qn.default_context().event_bracket_overhead_ms()
    for shape in a.shapes:
        indptr, cols, vals = SHAPES[shape]()
        n, nnz = indptr.size - 1, vals.size
        rng = np.random.default_rng(5)
        b, x0 = rng.standard_normal(n), np.zeros(n)
        model = 12 * nnz + 4 * (n + 1) + 24 * n
        model_mv = 12 * nnz + 4 * (n + 1) + 16 * n
        obj = qn.SparseQuadratic(indptr, cols, vals, b)
        auto = obj.lanes_per_row
        for lanes in a.lanes:
            obj.set_lanes_per_row(lanes)
            us, cnt = kernel_time_us(qn, obj, x0, a.iters, bracket_ms)
            line = dict(shape=shape, n=n, nnz=nnz, lanes=lanes, lanes_used=obj.lanes_per_row, auto_lanes=auto, long_rows=obj.n_long_rows,
                        eval_kernel_us=us, launches_timed=cnt, model_bytes=model, tb_per_s=model / (us * 1e-6) / 1e12 if us else None)
            print(json.dumps(line), flush=True)
        # the yardstick, and whole iterations with the automatic choice
        obj.set_lanes_per_row(0)
        us, _ = kernel_time_us(qn, obj, x0, a.iters, bracket_ms)
        summary = dict(shape=shape, n=n, nnz=nnz, summary=True, default_lanes=obj.lanes_per_row, default_eval_kernel_us=us,
                       default_tb_per_s=model / (us * 1e-6) / 1e12, model_ratio=model / model_mv)
        try:
            x = rng.standard_normal(n)
            t_us, y = torch_mv_us(indptr, cols, vals, x)
            _, g = obj(x)
            summary.update(torch_mv_us=t_us, torch_mv_tb_per_s=model_mv / (t_us * 1e-6) / 1e12, torch_mv_us_times_ratio=t_us * model / model_mv,
                           max_abs_diff_against_torch=float(np.max(np.abs((g + b) - y))))
        except Exception as e:  # noqa: BLE001 -- a build without sparse CSR mv: say so, no yardstick column
            summary.update(torch_mv="unavailable: " + repr(e)[:200])
        s = qn.LBFGS(0.0, x0, m=5, memoize=1)
        _minimize(qn, s, qn.StrongWolfe(1e-4, 0.9), obj, 2)
        s.reset(x0)
        dt = _minimize(qn, s, qn.StrongWolfe(1e-4, 0.9), obj, a.iters)
        summary.update(lbfgs_device_ms_per_iter=1e3 * dt / a.iters, lbfgs_device_evals=s.stats()["oracle_evals"])
        s.close()
        fn = host_closure(indptr, cols, vals, b)
        s = qn.LBFGS(0.0, x0, m=5, memoize=1)
        dt = _minimize(qn, s, qn.StrongWolfe(1e-4, 0.9), fn, a.host_iters)
        summary.update(lbfgs_host_closure_ms_per_iter=1e3 * dt / a.host_iters, lbfgs_host_closure_evals=s.stats()["oracle_evals"])
        s.close()
        obj.close()
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
