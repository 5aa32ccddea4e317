"""NewtonCG's Jacobi preconditioner and the Hessian-diagonal kernels (csrc/qn_hess_diag.hip.h, slog_diag_kernel).  Not run by any test.

  * --profile: nothing is timed here; the process makes REPS x (hess_vec_at, hess_diag_at) per shape behind a warm-up, for ONE profiled call
        rocprofv3 --kernel-trace --stats -- python tools/bench_precond.py --profile
    whose per-kernel statistics put hd_onepass_kernel beside lse_hv_onepass_kernel on the same dense A (m = n = 4096, 8192, 16384) and slog_diag_kernel
    beside slog_cols_kernel<.., true> on the same CSR pair (m = n = 2^20, 16 nonzeros per row).  Both calls start with the same weights pass, so the
    kernels alternate on one state of the machine.
  * default: whole runs of NewtonCG + BackTracking(1e-4, 0.5) with preconditioner "none" and "jacobi", ALTERNATING, on those shapes with the columns
    scaled by 10^U(-1.5, 1.5), mu = 1e-3, x0 = 0, to ||g||_inf < 1e-6 (at most MAX_OUTER outer iterations): outer iterations, inner total, wall
    milliseconds of `minimize` (median over REPS), and whether the run converged.  One JSON line per shape.
usage: bench_precond.py [--profile] [--dense n ...] [--no-sparse]"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

qn = ge.load_package()

REPS = 2
PROFILE_REPS = 5
MAX_OUTER = 100
TOL = 1e-6
MU = 1e-3
SPREAD = 1.5
SPARSE_N = 1 << 20
PER_ROW = 16
profile_only = "--profile" in sys.argv
args = sys.argv[1:]
dense_sizes = [4096, 8192, 16384]
if "--dense" in args:
    dense_sizes = [int(a) for a in args[args.index("--dense") + 1:] if not a.startswith("--")]
with_sparse = "--no-sparse" not in args


def dense_problem(n, scaled):
    rng = np.random.default_rng(33)
    a = rng.standard_normal((n, n))
    xs = rng.standard_normal(n) / np.sqrt(n)
    y = np.where(a @ xs + 0.3 * rng.standard_normal(n) >= 0.0, 1.0, -1.0)
    if scaled:
        a *= 10.0 ** rng.uniform(-SPREAD, SPREAD, n)
    return a, y


def sparse_problem(n, scaled):
    """PER_ROW entries per row, one drawn from each of PER_ROW equal strata of the columns: distinct and increasing"""
    rng = np.random.default_rng(34)
    width = n // PER_ROW
    cols = (np.arange(PER_ROW) * width)[None, :] + rng.integers(0, width, size=(n, PER_ROW))
    data = rng.standard_normal((n, PER_ROW))
    xs = rng.standard_normal(n) / np.sqrt(PER_ROW)
    y = np.where(np.sum(data * xs[cols], axis=1) + 0.3 * rng.standard_normal(n) >= 0.0, 1.0, -1.0)
    if scaled:
        data = data * (10.0 ** rng.uniform(-SPREAD, SPREAD, n))[cols]
    indptr = (np.arange(n + 1) * PER_ROW).astype(np.int64)
    return indptr, cols.reshape(-1).astype(np.int64), np.ascontiguousarray(data.reshape(-1)), y


def whole_runs(obj, n):
    out = {}
    x0 = np.zeros(n)
    rows = dict(none=[], jacobi=[])
    for rep in range(REPS + 1):  # (the first pair is the warm-up)
        for pc in ("none", "jacobi"):  # alternating: both settings see the same state of the machine
            s = qn.NewtonCG(TOL, x0, preconditioner=pc)
            qn.default_context().synchronize()
            t0 = time.perf_counter()
            status = "ok"
            try:
                s.minimize(qn.BackTracking(1e-4, 0.5), obj, MAX_OUTER, 30)
            except qn.MaxIterReached:
                status = "max_iter"
            qn.default_context().synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                rows[pc].append(dict(ms=ms, outer=s.k(), inner=s.inner_iterations()[1], status=status, diag_passes=s.diag_passes()))
            s.close()
    for pc, rs in rows.items():
        out[pc] = dict(outer=rs[0]["outer"], inner_total=rs[0]["inner"], status=rs[0]["status"], diag_passes=rs[0]["diag_passes"],
                       ms=[round(r["ms"], 2) for r in rs], ms_median=round(float(np.median([r["ms"] for r in rs])), 2))
    return out


def profile_calls(obj, n):
    rng = np.random.default_rng(35)
    x, v = 0.01 * rng.standard_normal(n), rng.standard_normal(n)
    obj.hess_vec_at(x, v, download=False)  # warm-up: code objects, the LDS attribute
    obj.hess_diag_at(x)
    for _ in range(PROFILE_REPS):
        obj.hess_vec_at(x, v, download=False)
        obj.hess_diag_at(x)


for n in dense_sizes:
    a, y = dense_problem(n, not profile_only)
    obj = qn.Logistic(a, y, MU)
    del a
    if profile_only:
        profile_calls(obj, n)
        print(f"dense n={n} profile: {PROFILE_REPS} x (hess_vec_at, hess_diag_at) on Logistic", flush=True)
    else:
        print(json.dumps(dict(kind="dense", m=n, n=n, mu=MU, tol=TOL, spread=SPREAD, bytes_per_pass=8 * n * n, **whole_runs(obj, n))), flush=True)
    obj.close()
if with_sparse:
    n = SPARSE_N
    ip, ix, data, y = sparse_problem(n, not profile_only)
    obj = qn.SparseLogistic(ip, ix, data, y, MU, n)
    if profile_only:
        profile_calls(obj, n)
        print(f"sparse n={n} profile: {PROFILE_REPS} x (hess_vec_at, hess_diag_at) on SparseLogistic, lanes {obj.lanes}", flush=True)
    else:
        print(json.dumps(dict(kind="sparse", m=n, n=n, nnz=int(data.size), mu=MU, tol=TOL, spread=SPREAD, **whole_runs(obj, n))), flush=True)
    obj.close()
