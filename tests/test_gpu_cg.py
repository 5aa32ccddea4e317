"""GPU tests of nonlinear conjugate gradient (QN_NONLINEAR_CG: NonlinearCG; kernels csrc/qn_cg.hip.h) against the restatement tests/ref_cg.py.
Windows are licensed case by case by tests/test_ref_cg.py (three summation orders agree to 1e-11 inside them); the GPU is compared inside them at the
family's 1e-9 max(1, ||x||).

beta of the last iteration of a window is compared at 1e-9 max(1, |beta|) -- the licence ends a window also where the three orders' betas are more
than 1e-11 max(1, |beta|) apart, the same factor of 100 as for the iterates -- and exactly where the restatement has 0 (a restart is a decision,
licensed by the window).

The shape test's bound is derived in cg_cases.beta_bound and holds for ANY summation order; tests/test_ref_cg.py checks the derivation
against three orders on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import cg_cases as C
import ref_cg as RC
import sparse_cases as SC
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH_VECTOR, PATH_CG = 64, 2048
INF = float("inf")


def _ls(qn, kind):
    return qn.StrongWolfe(*C.WOLFE) if kind == "wolfe" else qn.BackTracking(1e-4, 0.5)


def _oracle(qn, oracle, n):
    if oracle == "host":
        return C.oracle_fn("host", n)[0]
    if oracle == "lse":
        a, c, mu, _ = C.lse_problem(n)
        return qn.LogSumExp(a, c, mu)
    q, b, _, _ = C.L.quad_problem(n)
    return qn.Quadratic(q, b)


def _gpu(qn, oracle, x0, variant, ls, iters, memoize=None, powell_nu=0.2, restart_every=0, max_ls=50, tol=C.TOL, solver=None):
    s = solver or qn.NonlinearCG(tol, x0, variant=variant, powell_nu=powell_nu, restart_every=restart_every, memoize=memoize)
    s.set_trace(iters, with_x=True)
    status = "ok"
    try:
        s.minimize(_ls(qn, ls), oracle, iters, max_ls)
    except qn.MaxIterReached:
        status = "max_iter"
    return s, status


def _window_ref(ref, w):
    return type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))


def _compare_cg(s, ref, w):
    """iterates, t, n_evals, ls_iters, gnorm (test_gpu_spg._compare), then `updated`, s_norm, restarts() and beta() of the window's last iteration"""
    _compare(s, _window_ref(ref, w), w)
    tr, _ = s.trace()
    assert [r["updated"] for r in tr] == ref.updated[:w]
    for k in range(w):
        assert abs(tr[k]["s_norm"] - ref.trace[k]["s_norm"]) <= 1e-9 * max(1.0, ref.trace[k]["s_norm"]), k
    assert s.restarts() == ref.updated[:w].count(0)
    b = ref.betas[w - 1]
    assert (s.beta() == 0.0) if b == 0.0 else abs(s.beta() - b) <= 1e-9 * max(1.0, abs(b)), (s.beta(), b)
    since = 0
    for u in ref.updated[:w]:
        since = since + 1 if u else 0
    assert s.since_restart() == since


@pytest.mark.parametrize("memoize", [0, 1])
@pytest.mark.parametrize("variant,oracle,ls,n", C.CASES)
def test_parity_window(qn, variant, oracle, ls, n, memoize):
    ref = C.ref_case(variant, oracle, ls, n)[0]
    w = C.window(variant, oracle, ls, n)
    assert w >= C.MIN_WINDOW
    _, x0 = C.oracle_fn(oracle, n)
    s, status = _gpu(qn, _oracle(qn, oracle, n), x0, variant, ls, w, memoize=memoize)
    assert status == "max_iter" and s.variant == variant
    _compare_cg(s, ref, w)
    assert s.stats()["path"] == PATH_VECTOR | PATH_CG


@pytest.mark.parametrize("name", ["tri", "arrow"])
def test_parity_sparse_quadratic(qn, name):
    """the CSR device objective at n = 2050 (Hager-Zhang + StrongWolfe), licensed here the way cg_cases.licence does"""
    n = 2050
    fn, x0 = SC.quadratic_fn(SC.matrix(name, n), SC.rhs(n)), SC.start(n)
    ref, w, worst = C.licence_of(fn, x0, "hz", "wolfe")
    assert w >= C.MIN_WINDOW and worst <= C.LICENCE, (w, worst)
    indptr, cols, vals = SC.matrix(name, n)
    obj = qn.SparseQuadratic(indptr.astype(np.int32), cols.astype(np.int32), vals, SC.rhs(n))
    s, status = _gpu(qn, obj, x0, "hz", "wolfe", w)
    assert status == "max_iter"
    _compare_cg(s, ref, w)
    assert s.stats()["path"] == PATH_VECTOR | PATH_CG


# ---- the two kernels' shapes: beta of the second iteration against longdouble sums of the same vectors ----
@pytest.mark.parametrize("n", C.SHAPE_SIZES)
def test_beta_against_extended_precision(qn, n):
    """n = 2, 7, 4099 (three workgroups, a ragged last one), 2^21 + 3 (the grid-stride loop wraps).  One iteration, then one more: d_1 is rebuilt on the
    host from the GPU's own beta_1 with the kernel's two roundings (or its branch to -g), g_1 and g_2 are the closure's values at the traced iterates, so the sums of
    the second iteration's beta are taken over the vectors the accept kernel held, bit for bit.  Powell's test is off: the formula is what is measured."""
    fn, x0 = C.oracle_fn("host", n)
    for variant in RC.VARIANTS:
        s, status = _gpu(qn, fn, x0, variant, "wolfe", 1, powell_nu=INF)
        assert status == "max_iter"
        x1, beta1 = s.x(), s.beta()
        assert s.trace()[1][0].tobytes() == x1.tobytes()
        g0, g1 = fn(np.asarray(x0, dtype=np.float64))[1], fn(x1)[1]
        d1 = beta1 * (-g0) - g1 if beta1 != 0.0 else -g1  # (n = 2: PR+ and HS+ truncate the first beta to 0, and the kernel branches to -g)
        assert s.restarts() == (0 if beta1 != 0.0 else 1)
        _, status = _gpu(qn, fn, None, variant, "wolfe", 1, solver=s)
        assert status == "max_iter"
        x2 = s.x()
        tr, _ = s.trace()
        # x2 = fl(x1 + fl(t d1)) element by element: d1 IS the direction searched
        assert np.array_equal(x2, x1 + tr[0]["t"] * d1)
        exact, mags = C.ld_sums(g1, fn(x2)[1], d1)
        centre, bound = C.beta_bound(variant, n, exact, mags)
        assert -exact["gpgp"] + centre * exact["gpd"] < -1e-6 * exact["gpgp"]  # the descent guard is far from deciding
        print(f"n={n} {variant}: beta_gpu={s.beta():.17e} longdouble={centre:.17e} |diff|={abs(s.beta() - centre):.3e} bound={bound:.3e}")
        assert abs(s.beta() - centre) <= bound, (variant, s.beta(), centre, bound)
        assert tr[0]["updated"] == 1 and s.beta() != 0.0 and s.restarts() == (0 if beta1 != 0.0 else 1)


# ---- the same bits ----
@pytest.mark.parametrize("variant,oracle,ls,n", [("hz", "lse", "wolfe", 2050), ("fr", "host", "bt", 2050), ("pr+", "quad", "wolfe", 2050), ("dy", "lse", "bt", 7)])
def test_same_bits(qn, variant, oracle, ls, n):
    w = C.window(variant, oracle, ls, n)
    k = w // 2
    _, x0 = C.oracle_fn(oracle, n)
    o = _oracle(qn, oracle, n)
    one, _ = _gpu(qn, o, x0, variant, ls, 2 * k)
    again, _ = _gpu(qn, o, x0, variant, ls, 2 * k)
    assert one.trace()[1].tobytes() == again.trace()[1].tobytes() and one.beta() == again.beta()
    # two calls of k iterations are one call of 2 k: the direction, beta and the counters survive a call
    two, _ = _gpu(qn, o, x0, variant, ls, k)
    first = two.trace()[1].copy()
    _gpu(qn, o, None, variant, ls, k, solver=two)
    assert np.concatenate([first, two.trace()[1]]).tobytes() == one.trace()[1].tobytes()
    assert (two.beta(), two.restarts(), two.since_restart()) == (one.beta(), one.restarts(), one.since_restart())
    # qn_solver_reset gives the first run again (the variant is a setting: kept)
    two.reset(x0)
    assert (two.beta(), two.restarts(), two.since_restart(), two.variant) == (0.0, 0, 0, variant)
    _gpu(qn, o, None, variant, ls, 2 * k, solver=two)
    assert two.trace()[1].tobytes() == one.trace()[1].tobytes() and two.restarts() == one.restarts()


# ---- the restart rules ----
def test_first_direction_is_minus_g(qn):
    fn, x0 = C.oracle_fn("host", 4099)
    for variant in RC.VARIANTS:
        s, _ = _gpu(qn, fn, x0, variant, "wolfe", 1)
        tr, xs = s.trace()
        x0a = np.asarray(x0, dtype=np.float64)
        assert np.array_equal(xs[0], x0a + tr[0]["t"] * -fn(x0a)[1])  # t d == -t g, element by element
        assert s.restarts() == 0  # the first direction is no restart


def test_restart_every_third(qn):
    v, oracle, ls, n, nu, every = C.EVERY
    ref = C.ref_case(v, oracle, ls, n, "numpy", nu, every)[0]
    w = C.window(v, oracle, ls, n, nu, every)
    fn, x0 = C.oracle_fn(oracle, n)
    s, _ = _gpu(qn, fn, x0, v, ls, w, powell_nu=nu, restart_every=every)
    _compare_cg(s, ref, w)
    tr, xs = s.trace()
    assert [r["updated"] for r in tr] == [0 if k % 3 == 2 else 1 for k in range(w)] and s.restarts() == w // 3
    for k in range(3, w, 3):  # the direction after a restart is -g exactly
        assert np.array_equal(xs[k], xs[k - 1] + tr[k]["t"] * -fn(xs[k - 1])[1]), k
    assert not np.array_equal(xs[1], xs[0] + tr[1]["t"] * -fn(xs[0])[1])


def test_powell_nu_inf_removes_the_powell_restarts(qn):
    variant, oracle, ls, n = C.POWELL
    _, x0 = C.oracle_fn(oracle, n)
    o = _oracle(qn, oracle, n)
    on, off = C.ref_case(*C.POWELL)[0], C.ref_case(*C.POWELL, "numpy", INF)[0]
    w_on, w_off = C.window(*C.POWELL), C.window(*C.POWELL, INF)
    a, _ = _gpu(qn, o, x0, variant, ls, w_on)
    b, _ = _gpu(qn, o, x0, variant, ls, w_off, powell_nu=INF)
    _compare_cg(a, on, w_on)
    _compare_cg(b, off, w_off)
    assert "powell" in on.why[:w_on] and a.restarts() >= 1 and b.restarts() == 0


def test_set_cg_drops_p(qn):
    fn, x0 = C.oracle_fn("host", 2050)
    s, _ = _gpu(qn, fn, x0, "pr+", "wolfe", 3)
    x3 = s.x()
    assert s.beta() != 0.0
    s.set_cg("pr+", 0.2, 0)
    assert (s.beta(), s.since_restart()) == (0.0, 0)
    _gpu(qn, fn, None, "pr+", "wolfe", 1, solver=s)
    tr, xs = s.trace()
    assert np.array_equal(xs[0], x3 + tr[0]["t"] * -fn(x3)[1]) and s.restarts() == 0
    # ... where the same call without set_cg goes on along beta p - g
    c, _ = _gpu(qn, fn, x0, "pr+", "wolfe", 3)
    _gpu(qn, fn, None, "pr+", "wolfe", 1, solver=c)
    assert not np.array_equal(c.trace()[1][0], xs[0])
    s.set_cg("hz", INF, 7)
    assert s.variant == "hz"


def test_zero_beta_never_reads_a_stale_p(qn):
    """a constant gradient: y = 0, DY's 1 / 0 is not finite (rule 4) -- every direction is -g by the branch; FR's beta is 1 exactly"""
    c = np.array([1.0, -2.0, 0.5])
    fn = lambda x: (float(c @ x), c.copy())  # noqa: E731
    ref, _, _ = C.run_ref(fn, np.zeros(3), "dy", "bt", 3, powell_nu=INF)
    s, _ = _gpu(qn, fn, np.zeros(3), "dy", "bt", 3, powell_nu=INF)
    _compare(s, ref, 3)
    assert [r["updated"] for r in s.trace()[0]] == [0, 0, 0] and s.restarts() == 3 and s.beta() == 0.0
    ref, _, _ = C.run_ref(fn, np.zeros(3), "fr", "bt", 3, powell_nu=INF)
    s, _ = _gpu(qn, fn, np.zeros(3), "fr", "bt", 3, powell_nu=INF)
    _compare(s, ref, 3)
    assert s.beta() == 1.0 and s.restarts() == 0


# ---- synchronisation ----
@pytest.mark.parametrize("kind", ["sparse", "lse"])
def test_host_syncs_budget(qn, kind):
    n, w = 2050, 12
    if kind == "sparse":
        indptr, cols, vals = SC.matrix("tri", n)
        o, x0 = qn.SparseQuadratic(indptr.astype(np.int32), cols.astype(np.int32), vals, SC.rhs(n)), SC.start(n)
    else:
        o, x0 = _oracle(qn, "lse", n), C.oracle_fn("lse", n)[1]
    s = qn.NonlinearCG(C.TOL, x0, variant="hz")
    s.set_trace(w)
    before = s.stats()["host_syncs"]
    ks = []
    with pytest.raises(qn.MaxIterReached):
        s.minimize(_ls(qn, "wolfe"), o, w, 50, lambda r: ks.append(r.k()))
    st = s.stats()
    tr, _ = s.trace()
    extra = sum(r["ls_iters"] - 1 for r in tr)
    assert st["host_syncs"] - before <= w + extra + 2, (st["host_syncs"] - before, w, extra)  # one per iteration, one per further trial, a constant
    assert st["iterations"] == w and ks == list(range(1, w + 1)) and st["path"] == PATH_VECTOR | PATH_CG


def test_device_closure(qn):
    """the caller's own HIP objective (examples/device_closure.hip, the double-well chain) against the host closure of the same function"""
    import spg_cases as S
    from test_gpu_device_closure import _Chain
    a, c, x0, _, _ = S.chain_problem()
    ref, w, worst = C.licence_of(S.chain_fn(a, c), x0, "hz", "wolfe")
    assert w >= C.MIN_WINDOW and worst <= C.LICENCE, (w, worst)
    ch = _Chain(qn, a, c)
    try:
        for memoize in (0, 1):
            s, status = _gpu(qn, ch.closure, x0, "hz", "wolfe", w, memoize=memoize)
            assert status == "max_iter" and s.stats()["path"] == PATH_VECTOR | PATH_CG
            _compare_cg(s, ref, w)
    finally:
        ch.close()


# ---- rejections (host-side checks: no kernel runs) ----
def test_rejections(qn):
    n = 7
    fn, x0 = C.oracle_fn("host", n)
    s = qn.NonlinearCG(C.TOL, x0)
    assert (s.variant, s.beta(), s.restarts(), s.since_restart()) == ("pr+", 0.0, 0, 0)
    lb, ub = np.full(n, -1.0), np.full(n, 1.0)
    A = qn._abi
    dp = lambda v: v.ctypes.data_as(A.dp)  # noqa: E731
    assert A.lib().qn_solver_set_bounds(s.h, dp(lb), dp(ub)) == 3 and b"unbounded only" in A.lib().qn_last_error_message()
    g, d = np.ones(n), np.zeros(n)
    assert A.lib().qn_solver_compute_direction(s.h, dp(g), dp(d)) == 3 and b"use qn_minimize" in A.lib().qn_last_error_message()
    for ls, msg in ((qn.GLLQuadratic(1e-4, 10), "StrongWolfe or BackTracking"), (qn.BackTrackingB(1e-4, 0.5, lb, ub), "StrongWolfe or BackTracking"),
                    (qn.MoreThuente(), "StrongWolfe or BackTracking"), (qn.MoreThuenteB(n), "StrongWolfe or BackTracking")):
        with pytest.raises(qn.ErrorInputParams, match=msg):
            s.minimize(ls, fn, 5, 20)
    with pytest.raises(qn.ErrorInputParams, match="unknown variant"):
        s.set_cg("prp", 0.2, 0)
    assert A.lib().qn_solver_set_cg(s.h, 5, 0.2, 0) == 3 and b"unknown variant" in A.lib().qn_last_error_message()
    assert A.lib().qn_solver_set_cg(s.h, -1, 0.2, 0) == 3
    for nu in (0.0, -0.5, float("nan")):
        with pytest.raises(qn.ErrorInputParams, match="powell_nu must be positive"):
            s.set_cg("fr", nu, 0)
    assert s.variant == "pr+"  # a rejected call changes nothing
    s.set_cg("fr", INF, 4)
    assert s.variant == "fr"
    import ctypes
    assert A.lib().qn_solver_cg_state(s.h, None, None, None, None) == 0  # any pointer may be NULL
    other = qn.LBFGS(C.TOL, x0)
    assert A.lib().qn_solver_set_cg(other.h, 1, 0.2, 0) == 3 and b"NonlinearCG" in A.lib().qn_last_error_message()
    v = ctypes.c_int()
    assert A.lib().qn_solver_cg_state(other.h, ctypes.byref(v), None, None, None) == 3 and b"NonlinearCG" in A.lib().qn_last_error_message()
    # the solver still runs after all of that
    s.set_cg("pr+", 0.2, 0)
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.StrongWolfe(*C.WOLFE), fn, 2, 20)
    assert s.k() == 2


def test_examples_cg_cpp():
    exe = os.path.join(ROOT, "examples", "cg_example.bin")
    assert os.path.exists(exe), "examples/cg_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("||g||_inf") == 2 and p.stdout.strip().endswith("cg example ok")
