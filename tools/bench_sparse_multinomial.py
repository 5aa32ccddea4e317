"""Measures the sparse multinomial objective (qn.SparseMultinomial, csrc/qn_sparse_multinomial.hip.h).  Not run by any test.

Shapes: m = n = 2^20 with 16 uniformly random nonzeros per row at K = 4, 16 and 64 (rand20k4 / k16 / k64), a band of 16 per row at 2^20 with K = 16
(band20k16), and one shape the dense qn.Multinomial also takes: (65536, 1024, 16) at density 1 / 16 (dense16).  One JSON line per shape with
  * the evaluation's FOUR streaming kernels together (smn_in_kernel, smn_rows_kernel, smn_cols_kernel, smn_out_kernel: profiling mode brackets them
    under t_eval_ms, the one-workgroup finish counts under t_ctl_ms), minus the fixed part of an event bracket, over the evaluations of one
    LBFGS(5) + StrongWolfe call that continues a warm-up call, and model bytes / time in TB/s -- the model of qn_stats.obj_bytes:
    24 nnz + 4 (m + 1) + 4 (n + 1) + 24 m Kp + 32 n Kp + 24 K n + 12 m; the product's four the same way from a NewtonCG call (model with 8 m);
  * beside it, IN THE SAME PROCESS, qn.SparseLogistic's evaluation (its two streaming kernels) on the same pattern with its model
    24 nnz + 4 (m + 1) + 4 (n + 1) + 32 m + 24 n, the ratio of the two times (to be held against K: K binary passes would cost K times the second)
    and the ratio per model byte;
  * torch.sparse.mm on torch.sparse_csr_tensor for the two products alone, A Wt (n x K dense) and A' C (m x K dense);
  * at dense16, the dense qn.Multinomial's stream (its KC_EVAL bracket) on the densified matrix.
The bracket cannot tell the four kernels apart:
        rocprofv3 --kernel-trace --stats -- python tools/bench_sparse_multinomial.py --shapes rand20k16 --profile
gives each kernel's own time (a run of its own: --profile only launches evaluations and products).

    python tools/bench_sparse_multinomial.py [--shapes rand20k4 rand20k16 rand20k64 band20k16 dense16] [--iters 6] [--lanes 1 2 4 ...] [--profile]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"rand20k4": ("rand", 1 << 20, 1 << 20, 4), "rand20k16": ("rand", 1 << 20, 1 << 20, 16), "rand20k64": ("rand", 1 << 20, 1 << 20, 64),
          "band20k16": ("band", 1 << 20, 1 << 20, 16), "dense16": ("density", 65536, 1024, 16)}


def kp_of(k):
    return max(2, 1 << (k - 1).bit_length()) if k <= 16 else 16 * ((k + 15) // 16)


def torch_mm_us(a, dense, reps=10):
    import torch
    dev = torch.device("cuda")
    q = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int32)).to(dev), torch.from_numpy(a.indices.astype(np.int32)).to(dev),
                                torch.from_numpy(a.data).to(dev), size=a.shape, dtype=torch.float64, device=dev)
    d = torch.from_numpy(dense).to(dev)
    for _ in range(3):
        torch.sparse.mm(q, d)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        torch.sparse.mm(q, d)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--lanes", type=int, nargs="*", default=[])
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401 -- before libqn_hip.so is loaded, so that one HIP runtime serves both (tests/conftest.py says why)
    except ImportError:
        pass
    import __graft_entry__ as ge
    import bench_sparse_logistic as BL
    qn = ge.load_package()
    bracket_ms = qn.default_context().event_bracket_overhead_ms()
    mu = 0.5
    for shape in args.shapes:
        kind, m, n, k = SHAPES[shape]
        a = BL.random_rows(m, n) if kind == "rand" else BL.banded(m, n) if kind == "band" else BL.density(m, n, 1.0 / 16)
        nnz, kp = a.nnz, kp_of(k)
        rng = np.random.default_rng(5)
        y = rng.integers(0, k, size=m).astype(np.int32)
        x0, v = 0.01 * rng.standard_normal(k * n), rng.standard_normal(k * n)
        obj = qn.SparseMultinomial(a.indptr, a.indices, a.data, y, k, mu, n)
        if args.profile:
            for _ in range(4):
                obj(x0)
                obj.hess_vec_at(x0, v, download=False)
            print(f"{shape} profile: 4 x (evaluation, hess_vec_at) on SparseMultinomial")
            obj.close()
            continue
        common = 24 * nnz + 4 * (m + 1) + 4 * (n + 1) + 24 * m * kp + 32 * n * kp + 24 * k * n
        model_eval, model_prod = common + 12 * m, common + 8 * m
        out = dict(shape=shape, m=m, n=n, k=k, kp=kp, nnz=nnz, lanes=obj.lanes, long_rows=obj.n_long_rows, long_cols=obj.n_long_cols,
                   bracket_overhead_ms=round(bracket_ms, 5), model_eval_bytes=model_eval, model_product_bytes=model_prod, runs="one run")
        us, cnt = BL.eval_pair_us(qn, obj, x0, args.iters, bracket_ms)
        out.update(eval_four_kernels_us=us, eval_brackets_timed=cnt, eval_tb_per_s=model_eval / (us * 1e-6) / 1e12 if us else None)
        for lanes in args.lanes:
            obj.set_lanes(lanes, lanes)
            lus, _ = BL.eval_pair_us(qn, obj, x0, args.iters, bracket_ms)
            print(json.dumps(dict(shape=shape, lanes_forced=lanes, eval_four_kernels_us=lus, eval_tb_per_s=model_eval / (lus * 1e-6) / 1e12)), flush=True)
        obj.set_lanes(0, 0)
        pus, pcnt = BL.product_pair_us(qn, obj, x0, 2, bracket_ms)
        out.update(product_four_kernels_us=pus, product_brackets_timed=pcnt, product_tb_per_s=model_prod / (pus * 1e-6) / 1e12 if pus else None)
        obj.close()
        # SparseLogistic's evaluation on the same pattern, in the same process
        slog = qn.SparseLogistic(a.indptr, a.indices, a.data, np.where(y % 2 == 0, 1.0, -1.0), mu, n)
        sus, _ = BL.eval_pair_us(qn, slog, x0[:n].copy(), args.iters, bracket_ms)
        slog.close()
        smodel = 24 * nnz + 4 * (m + 1) + 4 * (n + 1) + 32 * m + 24 * n
        out.update(sparse_logistic_eval_us=sus, sparse_logistic_model_bytes=smodel, sparse_logistic_tb_per_s=smodel / (sus * 1e-6) / 1e12,
                   eval_over_sparse_logistic=us / sus, k_binary_passes_over_eval=k * sus / us, eval_per_byte_over_sparse_logistic=(us / model_eval) / (sus / smodel))
        try:
            t_a = torch_mm_us(a, rng.standard_normal((n, k)))
            t_at = torch_mm_us(a.T.tocsr(), rng.standard_normal((m, k)))
            out.update(torch_sparse_mm_a_wt_us=t_a, torch_sparse_mm_at_c_us=t_at, torch_sparse_mm_both_us=t_a + t_at)
        except Exception as e:  # noqa: BLE001 -- a build without sparse CSR mm: say so, no yardstick column
            out.update(torch_sparse_mm="unavailable: " + repr(e)[:200])
        if shape == "dense16":  # the dense objective on the densified matrix
            dense = qn.Multinomial(a.toarray(), y, k, mu)
            dus, _ = BL.eval_pair_us(qn, dense, x0, args.iters, bracket_ms)
            out.update(dense_multinomial_stream_us=dus, dense_multinomial_kernel=("mfma" if k > 16 else "vector"), dense_bytes=8 * m * n)
            dense.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
