"""The cases tests/test_gpu_run_plan.py pins and tests/golden/make_run_plan_pins.py records: one short run per branch of the host's run plan
(csrc/qn_host_minimize.hip.h: plan_run, plan_s2_args, the four pumps, finish_stats; csrc/qn_host_vec.hip.h for the first-order family), each at
the smallest shape that reaches the branch -- the second-generation path needs n == n_pad >= 8 * 128, its pair / ring / touch instances nb = 32
(n = 4096).  A case is a function of the product package that returns one record per minimize call: the qn_stats fields a moved launch, a moved
synchronisation or a changed byte formula would change, and the SHA-256 of x's bytes.  One module for the generator and the test: they cannot
diverge."""
import hashlib

import numpy as np

import problems as P

STAT_FIELDS = ("path", "launches", "host_syncs", "iterations", "oracle_calls", "oracle_evals", "h_passes", "h_bytes", "obj_bytes",
               "matrix_bytes_per_pass")
BOX = 0.05  # (the solution's entries are ~ b_i / Q_ii: a box of +-0.05 is active on a good part of them)

_objectives = {}


def quadratic(qn, n):
    """the seeded synthetic quadratic of tests/problems.py, generated on the device; one per size for the whole session"""
    if n not in _objectives:
        b, _ = P.synth_vectors(n)
        _objectives[n] = qn.Quadratic.synthetic(n, P.SEED, P.synth_diag(n), b)
    return _objectives[n]


def x0_of(n):
    return P.synth_vectors(n)[1]


def box(n):
    return np.full(n, -BOX), np.full(n, BOX)


def record(qn, s, call):
    """run one minimize call, return its record"""
    status = "Ok"
    try:
        call()
    except qn.SolverError as e:
        status = type(e).__name__
    st = s.stats()
    rec = {k: int(st[k]) for k in STAT_FIELDS}
    rec["status"] = status
    rec["x_sha256"] = hashlib.sha256(np.ascontiguousarray(s.x(), dtype=np.float64).tobytes()).hexdigest()
    return rec


def _unbounded(method, lsname, n, iters, options=(), sync=None, calls=1):
    def run(qn):
        s = getattr(qn, method)(1e-10, x0_of(n))
        for name, value in options:
            s.set_option(name, value)
        if sync is not None:
            s.set_sync_mode(sync)
        ls = qn.MoreThuente() if lsname == "mt" else qn.BackTracking(1e-4, 0.5)
        obj = quadratic(qn, n)
        return [record(qn, s, lambda: s.minimize(ls, obj, iters, 20)) for _ in range(calls)]
    return run


def _bounded(method, lsname, n, iters, options=(), calls=1):
    def run(qn):
        lb, ub = box(n)
        s = getattr(qn, method).new(1e-10, x0_of(n), lb, ub)
        for name, value in options:
            s.set_option(name, value)
        if lsname == "mtb":
            ls = qn.MoreThuenteB.new(n).with_lower_bound(lb).with_upper_bound(ub)
        elif lsname == "btb":
            ls = qn.BackTrackingB.new(1e-4, 0.5, lb, ub)
        else:
            ls = qn.MoreThuente()
        obj = quadratic(qn, n)
        return [record(qn, s, lambda: s.minimize(ls, obj, iters, 20)) for _ in range(calls)]
    return run


def _host_closure_with_callback(qn):
    n = 64
    d = P.synth_diag(n)
    b, x0 = P.synth_vectors(n)
    seen = []
    s = qn.BFGS(1e-10, x0)
    fn = lambda x: (float(np.sum(0.5 * d * x * x - b * x)), d * x - b)  # noqa: E731  (elementwise: the same bits wherever it runs)
    rec = record(qn, s, lambda: s.minimize(qn.MoreThuente(), fn, 10, 20, lambda solver: seen.append(solver.k())))
    rec["callback_k"] = seen
    return [rec]


def _logsumexp(qn):
    rng = np.random.default_rng(21)
    m = n = 1024
    a = rng.standard_normal((m, n)) * (3.0 / np.sqrt(n))
    c = rng.standard_normal(m)
    x0 = rng.standard_normal(n)
    obj = qn.LogSumExp(a, c, 0.1)
    s = qn.BFGS(1e-10, x0)
    rec = record(qn, s, lambda: s.minimize(qn.MoreThuente(), obj, 15, 20))
    s.close()
    obj.close()
    return [rec]


def _newton(qn):
    n = 64
    s = qn.Newton(1e-8, x0_of(n))
    obj = quadratic(qn, n)
    return [record(qn, s, lambda: s.minimize(qn.MoreThuente(), obj, 20, 20))]


def _spg(qn):
    n = 1000
    lb, ub = box(n)
    obj = quadratic(qn, n)
    s = qn.SpectralProjectedGradient(1e-10, x0_of(n), obj, lb, ub)
    return [record(qn, s, lambda: s.minimize(qn.GLLQuadratic(1e-4, 10), obj, 20, 50))]


CASES = {
    "01_bfgs_mt_4096": _unbounded("BFGS", "mt", 4096, 20),  # the benchmark's path: pair + ring + touch, pipelined
    "02_bfgs_mt_4096_sync": _unbounded("BFGS", "mt", 4096, 20, sync=1),  # second-generation synchronous pump
    "03a_bfgs_mt_4096_tail_reduce": _unbounded("BFGS", "mt", 4096, 20, options=(("tail_reduce", 1),)),
    "03b_bfgs_mt_4096_folded_accept_reduce": _unbounded("BFGS", "mt", 4096, 20, options=(("folded_accept_reduce", 1),)),
    "04_dfp_bt_1024": _unbounded("DFP", "bt", 1024, 20),  # the general second-generation body, fixed slots
    "05_bfgsb_mtb_1024": _bounded("BFGSB", "mtb", 1024, 20),  # bounded prologues, the stored-direction launch
    "06_bfgsb_btb_4096": _bounded("BFGSB", "btb", 4096, 12),  # BackTrackingB, projection inside the evaluation kernel
    "07_bfgsb_btb_4096_proj_launch": _bounded("BFGSB", "btb", 4096, 12, options=(("btb_project_in_eval", 0),)),
    "08_sr1b_mt_1024": _bounded("SR1B", "mt", 1024, 20),  # SR1 on the second-generation path
    "09_bfgs_mt_1024_first_generation": _unbounded("BFGS", "mt", 1024, 20, options=(("second_generation", 0),)),
    "10_bfgs_mt_1024_row_kernels": _unbounded("BFGS", "mt", 1024, 20, options=(("symmetric_storage", 0),)),
    "11_bfgs_mt_1024_generic_pipelined": _unbounded("BFGS", "mt", 1024, 20, options=(("generic_kernels", 1),), sync=0),
    "12_bfgs_mt_1024_generic_sync": _unbounded("BFGS", "mt", 1024, 20, options=(("generic_kernels", 1),), sync=1),
    "13_bfgs_mt_200_padded": _unbounded("BFGS", "mt", 200, 20),  # padding: no symmetric path
    "14_bfgs_host_closure_callback_64": _host_closure_with_callback,
    "15_bfgs_mt_logsumexp_1024": _logsumexp,
    "16_newton_64": _newton,
    "17_gd_bt_200": _unbounded("GradientDescent", "bt", 200, 20),  # no update pass
    "18a_bfgs_mt_4096_two_calls": _unbounded("BFGS", "mt", 4096, 5, calls=2),  # the warm continuation
    "18b_bfgsb_mtb_1024_two_calls": _bounded("BFGSB", "mtb", 1024, 5, calls=2),  # ... bounded: slots hint, kept clip of t_max
    "19_spg_gll_1000": _spg,  # the first-order family: the shared oracle check and totals
}
