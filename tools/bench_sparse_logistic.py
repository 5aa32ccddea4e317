"""Measures the sparse logistic objective (qn.SparseLogistic, csrc/qn_sparse_logistic.hip.h).  Not run by any test.

Shapes: m = n = 2^20 and 2^22 with 16 uniformly random nonzeros per row (x and coef gathered from all over the Infinity Cache / HBM), and a banded
pattern of 16 per row at m = n = 2^22 (the gathers hit L2); `dense13` is m = n = 8192 at density 1 / 16 beside the dense qn.Logistic on the densified
matrix.  One JSON line per shape with
  * the evaluation's TWO streaming kernels together (slog_rows_kernel + slog_cols_kernel: profiling mode brackets the pair under t_eval_ms, the
    one-workgroup finish counts under t_ctl_ms), minus the fixed part of an event bracket, over the evaluations of one LBFGS(5) + StrongWolfe call that
    continues a warm-up call, and model bytes / time in TB/s -- model = 24 nnz + 4 (m + 1) + 4 (n + 1) + 32 m + 24 n; the product's pair the same way
    from a NewtonCG call (t_newton_ms; model with 24 m);
  * beside it, IN THE SAME PROCESS, spq_eval_kernel (qn.SparseQuadratic, tools/bench_sparse.py's random symmetric pattern of about the same nnz) with
    its model 12 nnz + 4 (n + 1) + 24 n, and the ratio of the two per model byte.  The bracket cannot tell the row pass from the column pass:
        rocprofv3 --kernel-trace --stats -- python tools/bench_sparse_logistic.py --shapes rand20 --profile
    gives each kernel's own time (a run of its own: --profile only launches);
  * torch.mv on torch.sparse_csr_tensor for A and for A' (A x and A'c only: model 12 nnz + 4 (rows + 1) + 8 (m + n) each);
  * whole NewtonCG + BackTracking and LBFGS(5) + StrongWolfe iterations (wall clock per iteration of one qn_minimize call) on the device objective, and
    the LBFGS ones on a scipy host closure of the same function (two n-vectors over the bus per evaluation).

`--lanes L ...` adds one line per L with the evaluation's pair timed with L lanes per row forced on both passes.

    python tools/bench_sparse_logistic.py [--shapes rand20 rand22 band22 dense13] [--iters 6] [--host-iters 3] [--lanes 1 2 4 ...] [--profile]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def random_rows(m, n, per_row=16, seed=7):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m, dtype=np.int64), per_row)
    cols = rng.integers(0, n, size=m * per_row, dtype=np.int64)
    a = sp.csr_matrix((rng.standard_normal(m * per_row), (rows, cols)), shape=(m, n))
    a.sum_duplicates()
    a.sort_indices()
    return a


def banded(m, n, per_row=16, seed=7):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m, dtype=np.int64), per_row)
    cols = (rows * n // m + np.tile(np.arange(per_row, dtype=np.int64) - per_row // 2, m)) % n
    a = sp.csr_matrix((rng.standard_normal(m * per_row), (rows, cols)), shape=(m, n))
    a.sum_duplicates()
    a.sort_indices()
    return a


def density(m, n, p, seed=7):
    import scipy.sparse as sp
    a = sp.random(m, n, density=p, format="csr", random_state=np.random.default_rng(seed), data_rvs=np.random.default_rng(seed + 1).standard_normal)
    a.sort_indices()
    return a


SHAPES = {"rand20": lambda: random_rows(1 << 20, 1 << 20), "rand22": lambda: random_rows(1 << 22, 1 << 22), "band22": lambda: banded(1 << 22, 1 << 22),
          "dense13": lambda: density(8192, 8192, 1.0 / 16)}


def _minimize(qn, s, ls, oracle, iters):
    qn.default_context().synchronize()
    t0 = time.perf_counter()
    try:
        s.minimize(ls, oracle, iters, 30)
    except qn.MaxIterReached:
        pass
    qn.default_context().synchronize()
    return time.perf_counter() - t0


def eval_pair_us(qn, obj, x0, iters, bracket_ms):
    """microseconds per KC_EVAL bracket (SparseLogistic: rows + cols; SparseQuadratic: spq_eval_kernel) over one profiled LBFGS call"""
    s = qn.LBFGS(0.0, x0, m=5, memoize=1)
    _minimize(qn, s, qn.StrongWolfe(1e-4, 0.9), obj, 3)
    before = s.stats()
    s.set_profiling(1)
    _minimize(qn, s, qn.StrongWolfe(1e-4, 0.9), obj, iters)
    st = s.stats()
    s.close()
    cnt = st["n_eval_timed"] - before["n_eval_timed"]
    return (1e3 * ((st["t_eval_ms"] - before["t_eval_ms"]) / cnt - bracket_ms), cnt) if cnt else (None, 0)


def product_pair_us(qn, obj, x0, iters, bracket_ms):
    s = qn.NewtonCG(0.0, x0)
    s.set_profiling(1)
    _minimize(qn, s, qn.BackTracking(1e-4, 0.5), obj, iters)
    st = s.stats()
    out = (1e3 * (st["t_newton_ms"] / st["n_newton_timed"] - bracket_ms), st["n_newton_timed"]) if st["n_newton_timed"] else (None, 0)
    s.close()
    return out


def torch_mv_us(a, x, reps=20):
    import torch
    dev = torch.device("cuda")
    q = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int32)).to(dev), torch.from_numpy(a.indices.astype(np.int32)).to(dev),
                                torch.from_numpy(a.data).to(dev), size=a.shape, dtype=torch.float64, device=dev)
    xv = torch.from_numpy(x).to(dev)
    for _ in range(3):
        torch.mv(q, xv)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        torch.mv(q, xv)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def host_closure(a, y, mu):
    at = a.T.tocsr()

    def fn(x):
        z = y * a.dot(x)
        e = np.exp(-np.abs(z))
        q = 1.0 + e
        s = np.where(z >= 0.0, e, 1.0) / q
        return float(np.sum(np.maximum(-z, 0.0) + np.log1p(e))) + 0.5 * mu * float(x @ x), at.dot(-(y * s)) + mu * x
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--lanes", type=int, nargs="*", default=[])
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401 -- before libqn_hip.so is loaded, so that one HIP runtime serves both (tests/conftest.py says why)
    except ImportError:
        pass
    import __graft_entry__ as ge
    import bench_sparse as BS
    qn = ge.load_package()
    bracket_ms = qn.default_context().event_bracket_overhead_ms()
    mu = 0.5
    for shape in args.shapes:
        a = SHAPES[shape]()
        m, n = a.shape
        nnz = a.nnz
        rng = np.random.default_rng(5)
        xs = rng.standard_normal(n) / 4.0
        y = np.where(a.dot(xs) + 0.5 * rng.standard_normal(m) >= 0.0, 1.0, -1.0)
        x0, v = 0.01 * rng.standard_normal(n), rng.standard_normal(n)
        obj = qn.SparseLogistic(a.indptr, a.indices, a.data, y, mu, n)
        obj(x0)
        obj.hess_vec_at(x0, v, download=False)
        if args.profile:
            for _ in range(4):
                obj(x0)
                obj.hess_vec_at(x0, v, download=False)
            print(f"{shape} profile: 4 x (evaluation, hess_vec_at) on SparseLogistic")
            obj.close()
            continue
        model_eval = 24 * nnz + 4 * (m + 1) + 4 * (n + 1) + 32 * m + 24 * n
        model_prod = model_eval - 8 * m
        out = dict(shape=shape, m=m, n=n, nnz=nnz, lanes=obj.lanes, long_rows=obj.n_long_rows, long_cols=obj.n_long_cols, bracket_overhead_ms=round(bracket_ms, 5),
                   model_eval_bytes=model_eval, model_product_bytes=model_prod)
        us, cnt = eval_pair_us(qn, obj, x0, args.iters, bracket_ms)
        out.update(eval_rows_plus_cols_us=us, eval_brackets_timed=cnt, eval_tb_per_s=model_eval / (us * 1e-6) / 1e12 if us else None)
        for lanes in args.lanes:
            obj.set_lanes(lanes, lanes)
            lus, _ = eval_pair_us(qn, obj, x0, args.iters, bracket_ms)
            print(json.dumps(dict(shape=shape, lanes_forced=lanes, eval_rows_plus_cols_us=lus, eval_tb_per_s=model_eval / (lus * 1e-6) / 1e12)), flush=True)
        obj.set_lanes(0, 0)
        pus, pcnt = product_pair_us(qn, obj, x0, 3, bracket_ms)
        out.update(product_rows_plus_cols_us=pus, product_brackets_timed=pcnt, product_tb_per_s=model_prod / (pus * 1e-6) / 1e12 if pus else None)
        if m == n and shape != "dense13":  # the yardstick in the same process: spq_eval_kernel on a random symmetric pattern of about the same nnz
            ip, ci, va = BS.random_symmetric(n) if shape.startswith("rand") else BS.laplacian(int(round(np.sqrt(n))))
            quad = qn.SparseQuadratic(ip, ci, va, rng.standard_normal(n))
            qus, _ = eval_pair_us(qn, quad, np.zeros(n), args.iters, bracket_ms)
            qmodel = 12 * va.size + 4 * (n + 1) + 24 * n
            out.update(spq_pattern="random_symmetric" if shape.startswith("rand") else "laplacian", spq_nnz=int(va.size), spq_eval_kernel_us=qus,
                       spq_tb_per_s=qmodel / (qus * 1e-6) / 1e12, eval_per_byte_over_spq=(us / model_eval) / (qus / qmodel),
                       product_per_byte_over_spq=(pus / model_prod) / (qus / qmodel) if pus else None)
            quad.close()
        try:
            t_a, t_at = torch_mv_us(a, v), torch_mv_us(a.T.tocsr(), rng.standard_normal(m))
            mv_model = 12 * nnz + 8 * (m + n)
            out.update(torch_mv_a_us=t_a, torch_mv_at_us=t_at, torch_mv_a_tb_per_s=(mv_model + 4 * (m + 1)) / (t_a * 1e-6) / 1e12,
                       torch_mv_at_tb_per_s=(mv_model + 4 * (n + 1)) / (t_at * 1e-6) / 1e12)
        except Exception as e:  # noqa: BLE001 -- a build without sparse CSR mv: say so, no yardstick column
            out.update(torch_mv="unavailable: " + repr(e)[:200])
        for name, make, ls in (("newton_cg_bt", lambda: qn.NewtonCG(0.0, x0), qn.BackTracking(1e-4, 0.5)),
                               ("lbfgs5_wolfe", lambda: qn.LBFGS(0.0, x0, m=5, memoize=1), qn.StrongWolfe(1e-4, 0.9))):
            s = make()
            _minimize(qn, s, ls, obj, 2)
            s.close()
            s = make()
            dt = _minimize(qn, s, ls, obj, args.iters)
            out[f"{name}_device_ms_per_iter"] = 1e3 * dt / max(s.k(), 1)
            out[f"{name}_device_evals"] = s.stats()["oracle_evals"]
            if name == "newton_cg_bt":
                out["newton_cg_inner_per_iter"] = s.inner_iterations()[1] / max(s.k(), 1)
            s.close()
        s = qn.LBFGS(0.0, x0, m=5, memoize=1)
        dt = _minimize(qn, s, qn.StrongWolfe(1e-4, 0.9), host_closure(a, y, mu), args.host_iters)
        out.update(lbfgs5_wolfe_host_closure_ms_per_iter=1e3 * dt / max(s.k(), 1), lbfgs5_wolfe_host_closure_evals=s.stats()["oracle_evals"])
        s.close()
        if shape == "dense13":  # the dense objective on the densified matrix
            dense = qn.Logistic(a.toarray(), y, mu)
            dense(x0)
            for name, o in (("sparse", obj), ("dense", dense)):
                times = []
                for _ in range(10):
                    t0 = time.perf_counter()
                    o(x0)
                    times.append((time.perf_counter() - t0) * 1e3)
                out[f"{name}_eval_call_ms_median"] = float(np.median(times))
                s = qn.NewtonCG(0.0, x0)
                dt = _minimize(qn, s, qn.BackTracking(1e-4, 0.5), o, 3)
                out[f"{name}_newton_cg_bt_ms_per_iter"] = 1e3 * dt / max(s.k(), 1)
                s.close()
            dus, _ = eval_pair_us(qn, dense, x0, args.iters, bracket_ms)
            out.update(dense_eval_kernel_us=dus, dense_bytes=8 * m * 16 * ((n + 15) // 16))
            dense.close()
        obj.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
