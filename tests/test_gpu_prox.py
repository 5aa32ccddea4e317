"""GPU tests of QN_SPECTRAL_PROXIMAL_GRADIENT (qn.SpectralProximalGradient; kernels csrc/qn_vec_prox.hip.h) against the restatement
tests/ref_prox.py and the rules of DESIGN.md section 34: the direction and the convergence measure bit for bit from (x, g, lambda) for all four
instances of prox_dir_kernel; whole runs bit for bit at n <= 2; l1 = 0 against SpectralProjectedGradient byte for byte; the scalar / vector and
no-box / infinite-box instances against each other; windows and whole runs against the restatement; warm restarts and set_l1; the
synchronisation budget, the memory and the refusals."""
import math

import numpy as np
import pytest

import logistic_cases as LC
import multinomial_cases as MC
import prox_cases as PC
import ref_prox as RP
import ref_spg as R
import sparse_cases as SC
import sparse_logistic_cases as SLC
import spg_cases as S
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
PATH_VECTOR, PATH_PROX = 64, 16384
SIZES = (1, 2, 3, 255, 256, 257, 1000, 4099)


def _ls(qn, kind):
    return qn.GLLQuadratic(1e-4, 10) if kind == "gll" else qn.BackTracking(1e-4, 0.5)


def _run(qn, s, ls, oracle, iters, max_ls=PC.MAX_LS, callback=None):
    try:
        s.minimize(ls, oracle, iters, max_ls, callback=callback)
    except qn.MaxIterReached:
        return "max_iter"
    return "ok"


# ---- 5. direction and measure, bit for bit ----
def _crafted(n, boxed, l1vec):
    """f = 1/2 sum q_j (x_j - c_j)^2 with, by j mod 8: 0 a tie u == tau; 1 x_j == 0 exactly, staying there; 2 an unpenalised column; 3 x_j == lb_j
    pushed outwards; 4 x_j == ub_j pushed outwards; 5 generic; 6 a tie u == -tau; 7 x = 1 with d = -1 exactly, so that lambda0 = 1 / ||d0||_inf = 1
    (every other |d0_j| < 1) -- and with_lambdas(1, 1) keeps lambda = 1, which keeps the ties ties."""
    rng = np.random.default_rng(100 + n)
    j = np.arange(n) % 8
    x0 = rng.uniform(-0.4, 0.4, n)
    c = rng.uniform(-0.5, 0.5, n)
    q = rng.uniform(0.5, 1.0, n)
    l1 = rng.uniform(0.0, 0.3, n)
    lb, ub = np.full(n, -0.5), np.full(n, 0.5)
    for k, (xv, cv, qv, lv) in {0: (0.25, 0.5, 1.0, 0.5), 1: (0.0, 0.125, 1.0, 0.5), 3: (-0.5, -1.2, 1.0, 0.125), 4: (0.5, 1.0, 1.0, 0.125),
                                6: (-0.25, -0.5, 1.0, 0.5), 7: (1.0, 0.0, 1.0, 0.0)}.items():
        x0[j == k], c[j == k], q[j == k], l1[j == k] = xv, cv, qv, lv
    # 5: entries that stay live under every penalty used here (|q c| > 0.5) and do not reach their limit in one step (q < 1); |d0| <= |g0| < 0.91
    live = j == 5
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    x0[live], c[live], q[live] = (sgn * rng.uniform(0.1, 0.4, n))[live], (sgn * rng.uniform(1.1, 1.4, n))[live], rng.uniform(0.5, 0.7, n)[live]
    l1[j == 2] = 0.0
    ub[j == 7] = 2.0
    if not l1vec:  # one scalar: the ties are kept (tau = 0.5), the unpenalised column is not
        l1 = np.full(n, 0.5)

    def fn(x):
        return 0.5 * float(np.sum(q * (x - c) ** 2)), q * (x - c)
    return fn, x0, (l1 if l1vec else 0.5), l1, (lb if boxed else None), (ub if boxed else None)


def _check_directions(qn, s, oracle, ls, l1, lb, ub, iters):
    """run `iters` iterations; every d_k and every trace gnorm against rule 1 and rule 2 in numpy, from the solver's own (x_k, g_k, lambda_k)"""
    seen = []

    def cb(sv):
        seen.append((sv.direction(), sv.x(), sv.gradient(), sv.lambda_()))
    s.set_trace(iters, with_x=True)
    _run(qn, s, ls, oracle, iters, callback=cb)
    tr, xs = s.trace()
    assert len(tr) == len(seen) >= 1
    checked = 0
    for k in range(1, len(seen)):
        d_k = seen[k][0]
        _, x_k, g_k, lam_k = seen[k - 1]
        assert xs[k - 1].tobytes() == x_k.tobytes()
        want, _ = RP.prox_direction(x_k, g_k, lam_k, l1, lb, ub)
        assert d_k.tobytes() == want.tobytes(), (k, np.flatnonzero(d_k != want)[:5])
        gn = float(np.max(np.abs(RP.measure(x_k, g_k, l1, lb, ub))))
        assert tr[k]["gnorm"] == gn, (k, tr[k]["gnorm"], gn)
        checked += 1
    return seen, tr, checked


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("boxed", [False, True])
@pytest.mark.parametrize("l1vec", [False, True])
def test_direction_and_measure_bit_for_bit(qn, n, boxed, l1vec):
    fn, x0, l1_arg, l1, lb, ub = _crafted(n, boxed, l1vec)
    s = qn.SpectralProximalGradient(1e-300, x0, fn, l1_arg, lb, ub, memoize=1)
    try:
        if n >= 8:
            assert s.lambda_() == 1.0
        s.with_lambdas(1.0, 1.0)
        # iteration 0 as well: x0, the closure's g0 and the constructor's lambda0
        xs0 = s.x()
        g0 = fn(xs0)[1]
        want0, _ = RP.prox_direction(xs0, g0, s.lambda_(), l1, lb, ub)
        if n >= 8:  # the data holds what the issue asks for
            u = xs0 - g0
            assert np.any(u == l1) and np.any(u == -l1) and np.any(xs0 == 0.0)
            if boxed:
                assert np.any(xs0 == lb) and np.any(xs0 == ub)
            if l1vec:
                assert np.any(l1 == 0.0)
        seen, tr, checked = _check_directions(qn, s, fn, qn.GLLQuadratic(1e-4, 10), l1, lb, ub, 5)
        assert seen[0][0].tobytes() == want0.tobytes()
        assert tr[0]["gnorm"] == float(np.max(np.abs(RP.measure(xs0, g0, l1, lb, ub))))
        if n >= 8:
            assert checked >= 3
            assert np.any(seen[-1][1] == 0.0)  # exact zeros in x
        st = s.stats()
        assert st["path"] & PATH_PROX and st["path"] & PATH_VECTOR
    finally:
        s.close()


def test_direction_and_measure_past_one_grid_trip(qn):
    """n = 2^20 + 3 on a tridiagonal SparseQuadratic: every thread of prox_dir_kernel and prox_trial_kernel takes more than one trip of the
    grid-stride loop (1024 workgroups x 256 threads x 2 entries = 2^19 per trip), the last trip ragged"""
    n = (1 << 20) + 3
    indptr, cols, vals = SC.tri(n)
    obj = qn.SparseQuadratic(indptr, cols, vals, SC.rhs(n))
    x0 = SC.start(n) - 1.0  # [-0.5, 0.5)
    x0[::11] = 0.0
    l1 = np.full(n, 0.3)
    l1[::5] = 0.0
    lb, ub = np.full(n, -0.45), np.full(n, 0.45)
    s = qn.SpectralProximalGradient(1e-300, x0, obj, l1, lb, ub)
    try:
        seen, tr, checked = _check_directions(qn, s, obj, qn.GLLQuadratic(1e-4, 10), l1, lb, ub, 3)
        assert checked == 2
        x = seen[-1][1]
        assert np.any(x == 0.0) and np.any(x == lb) and np.any(x == ub) and np.all(x >= lb) and np.all(x <= ub)
    finally:
        s.close()
        obj.close()


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_runs_bit_for_bit(qn, n):
    """n <= 2: every sum has one order, so the whole run -- F_k, the measure, t, x -- is the restatement's with ref_prox.seq_dot, bit for bit.  (This
    is the comparison that rejects h1 taken from p: tests/test_ref_prox.py::test_planted_fault_h1_from_p.)"""
    ref = PC.run_tiny(n)
    fn, _, _, x0, l1 = PC.tiny_problem(n)
    s = qn.SpectralProximalGradient(1e-12, x0, fn, l1)
    try:
        s.set_trace(PC.TINY_ITERS, with_x=True)
        _run(qn, s, qn.GLLQuadratic(1e-4, 1), fn, PC.TINY_ITERS)
        tr, xs = s.trace()
        assert len(tr) == len(ref.trace)
        for k, (a, b) in enumerate(zip(tr, ref.trace)):
            for key in ("f", "gnorm", "t", "n_evals", "ls_iters", "s_norm"):
                assert a[key] == b[key], (k, key, a[key], b[key])
            assert xs[k].tobytes() == ref.trace_x[k].tobytes(), k
        assert s.lambda_() == ref.lam
    finally:
        s.close()


# ---- 6. l1 = 0 is SPG, byte for byte ----
def _objective(qn, qo, kind):
    """(oracle, host fn, x0, closer)"""
    if kind == "quadratic":
        q, b, x0, _ = S.problem(qo, 257)
        obj = qn.Quadratic(q, b)
        return obj, x0, obj.close
    if kind == "closure":
        q, b, x0, _ = S.problem(qo, 64)
        return R.quadratic_fn(q, b), x0, lambda: None
    pr = SLC.problem(40, 65)
    obj = qn.SparseLogistic(pr["indptr"], pr["indices"], pr["data"], pr["y"], pr["mu"], 65, weights=pr["w"])
    return obj, pr["x0"], obj.close


def _bytes(s):
    tr, xs = s.trace()
    st = s.stats()
    recs = [tuple(r[k] for k in ("f", "gnorm", "t", "s_norm", "y_norm", "n_evals", "ls_iters", "ls_cases", "updated")) for r in tr]
    return (s.x().tobytes(), np.array([r[:5] for r in recs]).tobytes(), [r[5:] for r in recs], xs.tobytes(), s.lambda_(),
            st["oracle_calls"], st["oracle_evals"], st["iterations"])


@pytest.mark.parametrize("kind", ["quadratic", "closure", "sparse_logistic"])
@pytest.mark.parametrize("ls", PC.SEARCHES)
@pytest.mark.parametrize("box", [0.3, None])
@pytest.mark.parametrize("memoize", [0, 1])
def test_l1_zero_is_spg(qn, qo, kind, ls, box, memoize):
    oracle, x0, close = _objective(qn, qo, kind)
    n, iters = x0.size, 12
    try:
        lb, ub = S.bounds(n, box if box is not None else float("inf"))
        spg = qn.SpectralProjectedGradient(1e-10, x0, oracle, lb, ub, memoize=memoize)
        prox = qn.SpectralProximalGradient(1e-10, x0, oracle, 0.0, *((lb, ub) if box is not None else (None, None)), memoize=memoize)
        out = []
        for s in (spg, prox):
            s.set_trace(iters, with_x=True)
            _run(qn, s, _ls(qn, ls), oracle, iters)
            out.append(_bytes(s))
            s.close()
        assert out[0] == out[1]
        assert out[0][-1] == iters
    finally:
        close()


# ---- 7. the instances against each other ----
def test_instance_equivalence(qn, qo):
    """a scalar l1 and a constant vector; no box and an infinite box: the same bytes (four instances of prox_dir_kernel, two of prox_trial_kernel)"""
    n, iters = 1000, 15
    q, b, x0, _ = S.problem(qo, n)
    obj = qn.Quadratic(q, b)
    try:
        out = []
        for boxed in (False, True):
            for vec in (False, True):
                lb, ub = S.bounds(n, float("inf")) if boxed else (None, None)
                s = qn.SpectralProximalGradient(1e-10, x0, obj, np.full(n, 0.5) if vec else 0.5, lb, ub)
                s.set_trace(iters, with_x=True)
                _run(qn, s, qn.GLLQuadratic(1e-4, 10), obj, iters)
                out.append(_bytes(s))
                assert 0 < s.nonzeros() < n
                s.close()
        assert out[0] == out[1] == out[2] == out[3]
    finally:
        obj.close()


# ---- 8. windows against the restatement ----
def _device_objective(qn, qo, kind, shape):
    if kind == "quadratic":
        q, b, _, _ = S.problem(qo, shape[0])
        return qn.Quadratic(q, b)
    if kind == "logistic":
        a, y, w, mu, _, _ = LC.problem(*shape)
        return qn.Logistic(a, y, mu, weights=w)
    if kind == "sparse_logistic":
        pr = SLC.problem(*shape)
        return qn.SparseLogistic(pr["indptr"], pr["indices"], pr["data"], pr["y"], pr["mu"], shape[1], weights=pr["w"])
    a, y, w, k, mu, _, _ = MC.problem(*shape)
    return qn.Multinomial(a, y, k, mu, weights=w)


class _Window:
    def __init__(self, ref, w):
        self.trace, self.trace_x = ref.trace[:w], ref.trace_x[:w]


@pytest.mark.parametrize("kind,shape,ls", PC.WINDOW_CASES)
def test_window_against_ref_prox(qn, qo, kind, shape, ls):
    w = PC.WINDOWS[(kind, shape, ls)]
    ref = PC.run_ref(kind, shape, ls, qo)[0]
    obj = _device_objective(qn, qo, kind, shape)
    _, x0 = PC.smooth(kind, shape, qo)
    lb, ub = PC.box_of(kind, shape)
    s = qn.SpectralProximalGradient(PC.TOL, x0, obj, PC.l1_of(kind, shape), lb, ub)
    try:
        s.set_trace(w, with_x=True)
        assert _run(qn, s, _ls(qn, ls), obj, w) == "max_iter"
        _compare(s, _Window(ref, w), w)
        tr, xs = s.trace()
        for k in range(w):  # F_k = f + h0, the trace's f
            assert abs(tr[k]["f"] - ref.trace[k]["f"]) <= 1e-9 * max(1.0, abs(ref.trace[k]["f"])), k
        assert np.array_equal(xs[w - 1] == 0.0, ref.trace_x[w - 1] == 0.0)  # the zero pattern
        assert s.stats()["path"] & (PATH_PROX | PATH_VECTOR) == PATH_PROX | PATH_VECTOR
    finally:
        s.close()
        obj.close()


# ---- 9. whole runs under GLLQuadratic(1e-4, 10) to 1e-7 ----
@pytest.mark.parametrize("kind,m,n,boxed", PC.RUN_CASES)
def test_whole_run(qn, kind, m, n, boxed):
    """The GPU run converges within the restatement's own iteration count plus 10 % (rounded up: the margin is for summation order near the
    tolerance), to the restatement's zero pattern, at a point that passes rule 2 for the closure's own (f, g).
    MEASURED on one MI355X, iterations restatement / GPU, free then lb = 0 -- logistic: (96, 64) 69 / 69, 41 / 41; (40, 65) 58 / 58, 32 / 32;
    (257, 200) 111 / 111, 79 / 79 -- least squares: (96, 64) 31 / 31, 40 / 40; (40, 65) 299 / 275, 59 / 59; (257, 200) 46 / 46, 51 / 51; the
    nonzero counts are equal in all twelve (10 to 96 of 64 to 200).  DESIGN.md section 34 has the table."""
    ref, status = PC.run_whole(kind, m, n, boxed)
    assert status == "ok"
    fn, l1, x0 = PC.run_problem(kind, m, n)
    lb, ub = PC.run_box(n, boxed)
    cap = int(math.ceil(1.1 * len(ref.trace)))
    s = qn.SpectralProximalGradient(PC.RUN_TOL, x0, fn, l1, lb, ub)
    try:
        s.set_trace(cap)
        status = _run(qn, s, qn.GLLQuadratic(1e-4, 10), fn, cap)
        x = s.x()
        print(f"whole run {kind} ({m}, {n}) boxed={boxed}: restatement {len(ref.trace)} iterations, GPU {s.k()} ({status}); nonzeros {s.nonzeros()} / {np.count_nonzero(ref.x)}")
        assert status == "ok", (s.k(), len(ref.trace))
        assert np.array_equal(x == 0.0, ref.x == 0.0)
        assert s.has_converged(fn(x))
        assert s.nonzeros() == np.count_nonzero(ref.x)
        if boxed:
            assert x.min() == 0.0
        # F is RUN_MU-strongly convex: a point whose subdifferential holds a v with ||v||_inf < tol lies within ||v||_2^2 / (2 mu) <= n tol^2 / (2 mu) of
        # the minimum; both runs end at such a point
        f_ref = fn(ref.x)[0] + ref.penalty()
        assert abs(s.composite(fn(x)) - f_ref) <= n * PC.RUN_TOL ** 2 / (2.0 * PC.RUN_MU) + 1e-12 * abs(f_ref)
    finally:
        s.close()


# ---- 10. warm restart and set_l1 ----
def test_warm_restart_bit_for_bit(qn, qo):
    n = 512
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, 0.05)
    l1 = np.full(n, 0.4)
    l1[::3] = 0.0
    obj = qn.Quadratic(q, b)
    try:
        one = qn.SpectralProximalGradient(1e-10, x0, obj, l1, lb, ub)
        assert _run(qn, one, qn.GLLQuadratic(1e-4, 10), obj, 30) == "max_iter"
        two = qn.SpectralProximalGradient(1e-10, x0, obj, l1, lb, ub)
        ls = qn.GLLQuadratic(1e-4, 10)
        for _ in range(2):
            assert _run(qn, two, ls, obj, 15) == "max_iter" and two.k() == 15
        assert one.x().tobytes() == two.x().tobytes() and one.lambda_() == two.lambda_()
        two.reset(x0)
        assert two.lambda_() is None and np.array_equal(two.l1, l1)  # the penalty is a setting: kept
    finally:
        obj.close()


def test_set_l1_between_calls(qn):
    """the regularisation-path use on logistic (96, 64): l1 2 -> 1 after 5 iterations.  The memo is kept (no evaluation at x in the next call), the
    ring is cleared (the first search interpolates once, as the restatement's with an empty ring; with the old ring it would accept t = 1:
    tests/test_ref_prox.py::test_set_l1_clears_the_ring_and_it_shows), lambda is kept, and the run converges at the new penalty"""
    first, after = PC.run_restart(True)
    a, y, w, mu, x0, _ = LC.problem(*PC.RESTART_SHAPE)
    obj = qn.Logistic(a, y, mu, weights=w)
    s = qn.SpectralProximalGradient(PC.RUN_TOL, x0, obj, PC.RESTART_L1[0])
    try:
        ls = qn.GLLQuadratic(1e-4, 10)
        s.set_trace(len(after), with_x=True)
        assert _run(qn, s, ls, obj, PC.RESTART_K) == "max_iter"
        lam, x = s.lambda_(), s.x()
        s.set_l1(PC.RESTART_L1[1])
        assert s.lambda_() == lam and s.x().tobytes() == x.tobytes() and np.all(s.l1 == PC.RESTART_L1[1])
        assert _run(qn, s, ls, obj, len(after)) == "max_iter"
        tr, _ = s.trace()
        st = s.stats()
        assert (tr[0]["ls_iters"], tr[0]["n_evals"]) == (after[0]["ls_iters"], after[0]["n_evals"]) and after[0]["ls_iters"] == 2
        assert abs(tr[0]["t"] - after[0]["t"]) <= 1e-9 * after[0]["t"]
        assert abs(tr[0]["f"] - after[0]["f"]) <= 1e-9 * abs(after[0]["f"])  # F_k at the NEW penalty from the kept smooth f
        # every call of the reference's sequence that found its point evaluated: the loop top and the accepted point of every iteration -- the
        # first loop top among them, which a call without the memo would have had to evaluate
        assert st["oracle_calls"] - st["oracle_evals"] == 2 * len(after)
        s.set_x(s.x())  # drops the memo: the same call now pays for its first loop top
        assert _run(qn, s, ls, obj, 2) == "max_iter"
        st = s.stats()
        assert st["oracle_calls"] - st["oracle_evals"] == 2 * 2 - 1
        s.set_trace(0)
        s.minimize(ls, obj, 2000, PC.MAX_LS)  # Ok(()): converged at the new penalty
        ev = obj(s.x())
        assert s.has_converged(ev) and 0 < s.nonzeros() < s.n
        assert abs(s.penalty() - PC.RESTART_L1[1] * np.sum(np.abs(s.x()))) <= 1e-12 * s.penalty()
    finally:
        s.close()
        obj.close()


# ---- 11. budget and refusals ----
def test_sync_budget_path_and_counters(qn, qo):
    n, window = 2048, 30
    q, b, x0, _ = S.problem(qo, n)
    lb, ub = S.bounds(n, 0.05)
    obj = qn.Quadratic(q, b)
    s = qn.SpectralProximalGradient(1e-10, x0, obj, 0.2, lb, ub)
    try:
        s.set_trace(window)
        before = s.stats()["host_syncs"]
        assert _run(qn, s, qn.GLLQuadratic(1e-4, 10), obj, window) == "max_iter"
        st = s.stats()
        tr, _ = s.trace()
        extra = sum(r["ls_iters"] - 1 for r in tr)
        # SPG's bound: one synchronisation per iteration whose first trial is accepted, one more per further trial, and a constant
        assert st["host_syncs"] - before <= window + extra + 2, (st["host_syncs"] - before, extra)
        assert st["path"] & (PATH_PROX | PATH_VECTOR) == PATH_PROX | PATH_VECTOR and st["iterations"] == window
    finally:
        s.close()
        obj.close()


def test_memory_is_linear_in_n(qn):
    import torch
    n = 1 << 22
    x0 = np.full(n, 0.5)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()

    def fn(x):  # f = 1/2 ||x||^2
        return 0.5 * float(x @ x), x
    s = qn.SpectralProximalGradient(1e-6, x0, fn, np.full(n, 0.25), np.full(n, -1.0), np.full(n, 1.0))
    try:
        assert s.lambda_() == 2.0  # d0 = soft(0.5 - 0.5, 0.25) - 0.5 = -0.5
        free1, _ = torch.cuda.mem_get_info()
        # SPG's 16 n doubles and the penalty's vector; 24 leaves room for the allocator's granularity (an n x n matrix would be 2^22 n)
        assert free0 - free1 <= 24 * n * 8, (free0 - free1) / (n * 8)
        with pytest.raises(qn.ErrorInputParams):
            s.approx_inv_hessian()
    finally:
        s.close()


def test_refusals(qn):
    def fn(x):
        return 0.5 * float(x @ x), x
    x0 = np.array([0.5, -0.25, 0.125])
    lb, ub = -np.ones(3), np.ones(3)
    s = qn.SpectralProximalGradient(1e-8, x0, fn, 0.1, lb, ub)
    spg = qn.SpectralProjectedGradient(1e-8, x0, fn, lb, ub)
    try:
        launches, x = s.stats()["launches"], s.x()
        for ls in (qn.BackTrackingB(1e-4, 0.5, lb, ub), qn.StrongWolfe(), qn.ExactQuadratic(), qn.MoreThuente(), qn.MoreThuenteB(3), qn.NoSearch()):
            with pytest.raises(qn.ErrorInputParams):
                s.minimize(ls, fn, 5, 5)
        with pytest.raises(qn.ErrorInputParams):
            s.compute_direction((0.0, np.ones(3)))
        for bad in (-1.0, float("nan"), float("inf"), np.array([0.1, -0.1, 0.1]), np.array([0.1, np.nan, 0.1]), np.array([0.1, np.inf, 0.1]), np.ones(2)):
            with pytest.raises(qn.ErrorInputParams):
                s.set_l1(bad)
        assert np.all(s.l1 == 0.1)
        L = qn._abi.lib()
        with pytest.raises(qn.ErrorInputParams):
            qn.solver._check(L.qn_solver_set_l1(spg.h, None, 0.1))
        out = np.empty(3)
        with pytest.raises(qn.ErrorInputParams):
            qn.solver._check(L.qn_solver_get_l1(spg.h, out.ctypes.data_as(qn._abi.dp)))
        assert s.stats()["launches"] == launches and s.x().tobytes() == x.tobytes()
        # a solver that has not run yet: nothing was ever launched
        raw = object.__new__(qn.SpectralProximalGradient)
        qn.solver._SolverBase.__init__(raw, 1e-8, x0)
        with pytest.raises(qn.ErrorInputParams):
            raw.minimize(qn.StrongWolfe(), fn, 5, 5)
        with pytest.raises(qn.ErrorInputParams):
            raw.set_l1(-0.5)
        assert raw.stats()["launches"] == 0
        raw.close()
        # the spectral setters answer for this method
        lam = s.lambda_()
        s.with_lambdas(1e-2, 1e2)
        assert (s.lambda_min(), s.lambda_max()) == (1e-2, 1e2) and s.lambda_() == lam
    finally:
        s.close()
        spg.close()


def test_world_above_one_is_rejected(qn):
    from thread_ranks import run_ranks

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        with pytest.raises(qn.ErrorInputParams, match="one rank"):
            qn.SpectralProximalGradient(1e-6, np.zeros(32), lambda x: (0.0, x), 0.1, ctx=ctx)
        ctx.close()
        return True
    assert run_ranks(2, body, timeout=60.0) == [True, True]
