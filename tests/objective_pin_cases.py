"""The cases tests/test_gpu_objective_pins.py pins and tests/golden/make_objective_pins.py records: every device objective kind (csrc/: Quadratic,
LogSumExp, SparseQuadratic, Logistic, SparseLogistic, Multinomial) through every host entry point and one short run of every solver family, each
objective at the smallest shape that reaches its branches.  tests/run_plan_cases.py does the same for the dense family's run plan on Quadratic and
LogSumExp only; this module is its twin for the layer that chooses between the kinds.

A case is a function of the product package that returns a list of records.  An entry-point record is the SHA-256 of the returned bytes, or on
refusal the exception class and the FULL message; a solver record is run_plan_cases.record's (the qn_stats counters and byte totals, x bit for bit)
plus the message on refusal.  Every case builds its own objective and closes it: a case leaves the same records alone, first or last.
One module for the generator and the test: they cannot diverge."""
import ctypes
import functools
import hashlib

import numpy as np

import logistic_cases as LC
import lse_hess_vec_cases as HV
import multinomial_cases as MC
import run_plan_cases as RP
import sparse_cases as SC
import sparse_logistic_cases as SL

ITERS = 5
MAX_LS = 20
BOX = 1.0  # every bounded run: x0 clipped into +-BOX
TIMERS = ("t_hpass_ms", "t_eval_ms", "t_ctl_ms", "t_comm_ms", "t_hreduce_ms", "t_ereduce_ms", "t_newton_ms")
DOWNLOAD_LIMIT = 4096  # the n x n Hessian of a wider objective (2 GB at n = 16400) is computed, not brought back and hashed


# ---- the data: (constructor arguments, x0, v), computed once, read-only ----
@functools.lru_cache(maxsize=None)
def _dense_q(n, symmetric):
    """diagonally dominant, built entry by entry (no BLAS: the same bits on every host); the non-symmetric one differs in one entry"""
    rng = np.random.default_rng(200 + n)
    r = rng.uniform(-1.0, 1.0, (n, n)) / n
    q = 0.5 * (r + r.T)
    q[np.arange(n), np.arange(n)] = 1.0 + np.arange(n) / n
    if not symmetric:
        q[0, 1] += 1e-3
    b, x0, v = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    return q, b, x0, v


@functools.lru_cache(maxsize=None)
def _slog_2100():
    """2100 x 2100, about ten entries per row, plus one full row and one full column (longer than the 2048 that get a workgroup of their own)"""
    m = n = 2100
    rng = np.random.default_rng(SL.SEED_BASE * m + n)
    mask = rng.random((m, n)) < 0.005
    mask[7, :] = True
    mask[:, 3] = True
    a = np.where(mask, rng.standard_normal((m, n)), 0.0)
    y = np.where(rng.standard_normal(m) >= 0.0, 1.0, -1.0)
    w = rng.choice(SL.WEIGHT_VALUES, size=m)
    x0, v = 0.1 * rng.standard_normal(n), rng.standard_normal(n)
    indptr, indices, data = SL.to_csr(a, mask)
    return indptr, indices, data, y, w, x0, v


def _quadratic(symmetric):
    def make(qn):
        q, b, x0, v = _dense_q(200, symmetric)
        return qn.Quadratic(q, b), x0, v
    return make


def _logsumexp(m, n):
    def make(qn):
        a, c, mu, x0, v = HV.problem(m, n)
        return qn.LogSumExp(a, c, mu), x0, v
    return make


def _sparse_quadratic(qn):
    n = 2100
    indptr, indices, data = SC.arrow(n)  # tridiagonal plus a full first row and column
    return qn.SparseQuadratic(indptr, indices, data, SC.rhs(n)), SC.start(n), np.random.default_rng(n).standard_normal(n)


def _logistic(qn):
    a, y, w, mu, x0, v = LC.problem(300, 200)
    return qn.Logistic(a, y, mu, weights=w), x0, v


def _sparse_logistic(qn):
    indptr, indices, data, y, w, x0, v = _slog_2100()
    return qn.SparseLogistic(indptr, indices, data, y, SL.MU, 2100, weights=w), x0, v


def _multinomial(m, nf, k):
    def make(qn):
        a, y, w, k_, mu, x0, v = MC.problem(m, nf, k)
        return qn.Multinomial(a, y, k_, mu, weights=w), x0, v
    return make


OBJECTIVES = {
    "quadratic_sym_200": _quadratic(True),  # n != n_pad
    "quadratic_nonsym_200": _quadratic(False),  # q_symmetric false
    "logsumexp_300x200": _logsumexp(300, 200),  # one-pass evaluation
    "logsumexp_64x16400": _logsumexp(64, HV.TOO_WIDE),  # n_pad > 16384: two-pass evaluation, the product "not built"
    "sparse_quadratic_2100": _sparse_quadratic,  # one row longer than 2048, symmetric
    "logistic_300x200": _logistic,
    "sparse_logistic_2100x2100": _sparse_logistic,  # one long row and one long column
    "multinomial_k3_nf70": _multinomial(100, 70, 3),  # the vector-unit kernel
    "multinomial_k20_nf33": _multinomial(100, 33, 20),  # K > 16: the MFMA kernel by the automatic choice
}


# ---- records ----
def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def _entry(qn, call):
    """one host entry point: the hash of the bytes it returned (the integers of an info getter as they are), or the class and the whole text of its refusal"""
    try:
        return {"status": "Ok", "result": call()}
    except qn.SolverError as e:
        return {"status": type(e).__name__, "message": str(e)}


def _abi_probabilities(qn, obj, x0):
    """qn_multinomial_probabilities on any handle (the Python method lives on Multinomial only)"""
    m, k = getattr(obj, "m", 1), getattr(obj, "n_classes", 1)
    p = np.zeros((m, k))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    qn.solver._check(qn._abi.lib().qn_multinomial_probabilities(obj.h, dp(np.ascontiguousarray(x0)), dp(p)))
    return _sha(p)


def _entries(name):
    def run(qn):
        obj, x0, v = OBJECTIVES[name](qn)
        n = obj.n
        try:
            def hessian():
                if n > DOWNLOAD_LIMIT:
                    obj.hessian(x0, download=False)
                    return "not downloaded"
                return _sha(obj.hessian(x0))
            calls = [
                ("eval", lambda: (lambda fe: _sha([fe.f()], fe.g()))(obj(x0))),
                ("hess_vec", lambda: (lambda qc: _sha(qc[0], [qc[1]]))(obj.hess_vec(v))),
                ("hess_vec_at", lambda: (lambda qc: _sha(qc[0], [qc[1]]))(obj.hess_vec_at(x0, v))),
                ("hessian", hessian),
                ("get_rows", lambda: _sha(obj.rows(1, 3))),
                ("sparse_info", lambda: repr(tuple(int(i) for i in qn.SparseQuadratic._info(obj)))),
                ("sparse_logistic_info", lambda: repr(qn.SparseLogistic._info(obj))),
                ("probabilities", lambda: _abi_probabilities(qn, obj, x0)),
                ("eval_again", lambda: (lambda fe: _sha([fe.f()], fe.g()))(obj(x0))),  # (after the weights passes above: the trial buffers)
            ]
            return [dict(_entry(qn, call), entry=entry) for entry, call in calls]
        finally:
            obj.close()
    return run


def _bounds(x0):
    return np.full(x0.size, -BOX), np.full(x0.size, BOX), np.clip(x0, -BOX, BOX)


def _solver_run(qn, make_solver, make_ls, obj, calls=1, profiling=False, state=None):
    """`calls` minimize calls on one solver; a refusal -- at construction (SPG evaluates there) or in minimize -- is a record too"""
    try:
        s = make_solver()
    except qn.SolverError as e:
        return [{"status": type(e).__name__, "message": str(e), "at": "construction"}]
    try:
        if profiling:
            s.set_profiling(1)
        recs = []
        for _ in range(calls):
            message = []

            def call():
                try:
                    s.minimize(make_ls(), obj, ITERS, MAX_LS)
                except qn.SolverError as e:
                    message.append(str(e))
                    raise
            rec = RP.record(qn, s, call)
            if message and rec["status"] in ("ErrorInputParams", "AbnormalTermination"):
                rec["message"] = message[0]
            if profiling:
                st = s.stats()
                rec["timed"] = {k: bool(st[k] != 0.0) for k in TIMERS}
            if state:
                rec["state"] = [int(i) for i in state(s)]
            recs.append(rec)
        return recs
    finally:
        s.close()


def _run(name, kind):
    def run(qn):
        obj, x0, _ = OBJECTIVES[name](qn)
        lb, ub, xb = _bounds(x0)
        bt = lambda: qn.BackTracking(1e-4, 0.5)  # noqa: E731
        try:
            if kind == "spg_gll":
                return _solver_run(qn, lambda: qn.SpectralProjectedGradient(1e-10, xb, obj, lb, ub), lambda: qn.GLLQuadratic(1e-4, 10), obj)
            if kind == "spg_gll_profiled":
                return _solver_run(qn, lambda: qn.SpectralProjectedGradient(1e-10, xb, obj, lb, ub), lambda: qn.GLLQuadratic(1e-4, 10), obj,
                                   profiling=True)
            if kind == "lbfgs_wolfe_two_calls":  # the second call starts warm: the memo keyed on the objective's serial
                return _solver_run(qn, lambda: qn.LBFGS(1e-10, x0), qn.StrongWolfe, obj, calls=2)
            if kind == "cg_bt":
                return _solver_run(qn, lambda: qn.NonlinearCG(1e-10, x0), bt, obj)
            if kind == "lbfgs_exact":
                return _solver_run(qn, lambda: qn.LBFGS(1e-10, x0), qn.ExactQuadratic, obj,
                                   state=lambda s: (lambda e: (e["curvature_passes"], e["refreshes"]))(s.exact_state()))
            if kind == "newton_cg_bt":
                return _solver_run(qn, lambda: qn.NewtonCG(1e-10, x0, chunk=2), bt, obj, state=lambda s: s._tn_state())
            if kind == "newton_cg_bt_profiled":
                return _solver_run(qn, lambda: qn.NewtonCG(1e-10, x0, chunk=2), bt, obj, profiling=True, state=lambda s: s._tn_state())
            if kind == "bfgs_mt":
                return _solver_run(qn, lambda: qn.BFGS(1e-10, x0), qn.MoreThuente, obj)
            if kind == "newton_mt":
                return _solver_run(qn, lambda: qn.Newton(1e-10, x0), qn.MoreThuente, obj)
            if kind == "pnewton_btb":
                return _solver_run(qn, lambda: qn.ProjectedNewton.new(1e-10, xb, lb, ub), lambda: qn.BackTrackingB.new(1e-4, 0.5, lb, ub), obj)
            raise KeyError(kind)
        finally:
            obj.close()
    return run


RUNS = ("spg_gll", "spg_gll_profiled", "lbfgs_wolfe_two_calls", "cg_bt", "lbfgs_exact", "newton_cg_bt", "newton_cg_bt_profiled", "bfgs_mt",
        "newton_mt", "pnewton_btb")

CASES = {}
for _name in OBJECTIVES:
    CASES[_name + "/entries"] = _entries(_name)
    for _kind in RUNS:
        CASES[_name + "/" + _kind] = _run(_name, _kind)
