"""GPU tests of the StrongWolfe line search (QN_LS_STRONG_WOLFE; kernels csrc/qn_vec_wolfe.hip.h) on the vector-machine solvers, against the
restatement tests/ref_wolfe.py (MINPACK-2 dcsrch / dcstep).  Windows and the tolerance (1e-9 max(1, ||x||), the family's: DESIGN 21) are licensed
case by case by tests/test_ref_wolfe.py; the cases are tests/wolfe_cases.py's."""
import numpy as np
import pytest

import lbfgs_cases as LC
import pnewton_cases as PC
import ref_spg as R
import ref_wolfe as RW
import spg_cases as S
import wolfe_cases as W
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
PATH_VECTOR, PATH_PNEWTON, PATH_LBFGS = 64, 128, 1024
EPS = float(np.finfo(np.float64).eps)


def _ls(qn, case, boxed=None):
    n, box = case[2], case[4]
    kw = dict(case[5]) if len(case) > 5 else {}
    ls = qn.StrongWolfe(kw.get("c1", 1e-4), kw.get("c2", 0.9))
    if "t_max" in kw:
        ls.with_t_max(kw["t_max"])
    if box is not None if boxed is None else boxed:
        lb, ub = W.box_of(n, box)
        ls.with_lower_bound(lb).with_upper_bound(ub)
    return ls


class _Oracle:
    """what the GPU solver is handed for a case's oracle kind; close() frees a device closure"""

    def __init__(self, qn, case):
        oracle, n = case[1], case[2]
        self.chain = None
        if case[0] == "pn":
            a, c, mu, _, _, _ = S.lse_problem()
            self.o = PC.lse_hess_fn(a, c, mu)
        elif oracle == "chain":
            from test_gpu_device_closure import _Chain
            a, c, _, _, _ = S.chain_problem(n)
            self.chain = _Chain(qn, a, c)
            self.o = self.chain.closure
        elif oracle == "lse":
            a, c, mu = (S.lse_problem() if n == 64 else LC.lse_problem(n))[:3]
            self.o = qn.LogSumExp(a, c, mu)
        elif oracle == "quad":
            q, b, _, _ = LC.quad_problem(n)
            self.o = qn.Quadratic(q, b)
        else:
            self.o = W.problem(oracle, n)[0]

    def close(self):
        if self.chain:
            self.chain.close()


def _gpu(qn, case, oracle, iters, memoize=None, max_ls=W.MAX_LS, ls=None, callback=None):
    solver, _, n, m, box = case[:5]
    x0 = W.problem(case[1], n)[1]
    lb, ub = W.box_of(n, box)
    if solver == "lbfgs":
        s = qn.ProjectedLBFGS(W.TOL, x0, lb, ub, m=m, memoize=memoize)
    elif solver == "spg":
        s = qn.SpectralProjectedGradient(W.TOL, x0, oracle, lb, ub, memoize=memoize)
    else:
        s = (qn.ProjectedNewton if solver == "pn" else qn.ProjectedGradientDescent)(W.TOL, x0, lb, ub)
        s.memoize = memoize
    s.set_trace(iters, with_x=True)
    ls = ls or _ls(qn, case)
    status = "ok"
    try:
        s.minimize(ls, oracle, iters, max_ls, callback)
    except qn.MaxIterReached:
        status = "max_iter"
    return s, ls, status


def _compare_window(s, case, w):
    """iterates, t, the norm, ls_iters, n_evals (test_gpu_spg._compare), then ls_cases, updated and f per iteration.  The bound on f is
    test_gpu_lbfgs._compare_updates': ||g(x_k)||_2 times the licensed 1e-9 max(1, ||x_k||), plus 1e-11 max(1, |f|) for a device objective's own
    summation order."""
    ref, rls, _, _ = W.ref_case(case)
    ref_w = type("Ref", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
    _compare(s, ref_w, w)
    tr, _ = s.trace()
    fn, x0 = W.problem(case[1], case[2])
    for k in range(w):
        assert tr[k]["ls_cases"] == rls.history[k]["ls_cases"], (k, oct(tr[k]["ls_cases"]), oct(rls.history[k]["ls_cases"]))
        if case[0] == "lbfgs":
            assert tr[k]["updated"] == ref.updated[k], k
        xk = ref.trace_x[k - 1] if k else R.box_projection(np.asarray(x0, dtype=np.float64), ref.lb, ref.ub)
        fr = ref.trace[k]["f"]
        bound = 1e-9 * max(1.0, float(np.linalg.norm(xk))) * float(np.linalg.norm(fn(xk)[1])) + 1e-11 * max(1.0, abs(fr))
        assert abs(tr[k]["f"] - fr) <= bound, (k, tr[k]["f"], fr, bound)


@pytest.mark.parametrize("memoize", [0, 1])
@pytest.mark.parametrize("case", W.CASES + W.BOX_CASES, ids=str)
def test_parity_window(qn, case, memoize):
    w = W.window(case)
    o = _Oracle(qn, case)
    try:
        s, ls, status = _gpu(qn, case, o.o, w, memoize=memoize)
    finally:
        o.close()
    assert status == "max_iter"
    _compare_window(s, case, w)
    path = s.stats()["path"]
    assert path & PATH_VECTOR and bool(path & PATH_LBFGS) == (case[0] == "lbfgs") and bool(path & PATH_PNEWTON) == (case[0] == "pn")
    if case[4] is not None:  # the boxed form: nothing left the search's box, and the line-search value kept its t_max
        lb, ub = W.box_of(case[2], case[4])
        xs = s.trace()[1]
        assert np.all(xs >= lb) and np.all(xs <= ub) and ls.t_max() == 1e10


def test_n2_steps_are_bit_equal(qn):
    """n = 2 on a host closure: one thread holds both products, so the sums are the restatement's own (ref_wolfe.seq_dot) and every decision
    is taken from the same bits -- t is EQUAL in every iteration of the window"""
    case = ("pgd", "concave", 2, 0, None, W.TMAX8)
    w = W.window(case)
    ref, rls, _, _ = W.run_ref(case, dot=RW.seq_dot, iters=w)
    s, _, _ = _gpu(qn, case, LC.concave_mixed_fn, w)
    tr, xs = s.trace()
    assert len(tr) == w
    for k in range(w):
        assert tr[k]["t"] == ref.trace[k]["t"], (k, tr[k]["t"], ref.trace[k]["t"])
        assert tr[k]["ls_cases"] == rls.history[k]["ls_cases"] and xs[k].tobytes() == ref.trace_x[k].tobytes(), k
    assert any(len(h["steps"]) >= 2 and 4 in h["cases"] for h in rls.history)


@pytest.mark.parametrize("n", [2, 7, 4099, (1 << 21) + 3])
def test_phi_prime_at_the_kernels_shapes(qn, n):
    """n = 2; 7 (odd, padding); 4099 (G = 3, a ragged last workgroup); 2^21 + 3 (G capped at 1024: the grid-stride loop wraps).  Projected gradient on
    lbfgs_cases.separable_problem, a host closure: t = 1 overshoots (case 1), and a search capped at ONE trial returns the second t -- the first
    interpolated one -- which depends on the kernels' two sums g.d and gt.d and on f values that are the closure's own.
    Reference: both sums in longdouble on the host, pushed through dcstep.  Bound: a sum of n products accumulated in any order is within
    n eps sum|a_i b_i| of the exact one; t2 is evaluated at the four corners (g.d +- that, gt.d +- that) and may differ from the reference by the
    largest corner deviation (dcstep's case-1 formula is smooth and monotone in both on that box), doubled, plus 4 ulp of t2 for dcstep's own
    arithmetic."""
    fn, x0 = LC.separable_problem(n)
    lb, ub = LC.free_box(n)
    s = qn.ProjectedGradientDescent(W.TOL, x0, lb, ub)
    s.set_trace(1)
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.StrongWolfe(), fn, 1, 1)
    tr, _ = s.trace()
    assert tr[0]["ls_iters"] == 1 and tr[0]["ls_cases"] == 1
    f0, g0 = fn(x0)
    d = -g0
    f1, g1 = fn(x0 + 1.0 * d)
    dl = d.astype(np.longdouble)
    gd, dphi = float(np.sum(g0.astype(np.longdouble) * dl)), float(np.sum(g1.astype(np.longdouble) * dl))
    e0, e1 = n * EPS * float(np.sum(np.abs(g0 * d))), n * EPS * float(np.sum(np.abs(g1 * d)))

    def t2(a, b):
        m = RW.Dcsrch(1e-4, 0.9, 0.1, 0.0, 1e10)
        m.start(f0, a)
        task, case = m.step(f1, b)
        assert task == "FG" and case == 1
        return m.stp
    ref = t2(gd, dphi)
    bound = 2.0 * max(abs(t2(gd + u, dphi + v) - ref) for u in (-e0, e0) for v in (-e1, e1)) + 4 * EPS * ref
    print(f"n={n} t2={tr[0]['t']!r} ref={ref!r} diff={abs(tr[0]['t'] - ref):.3e} bound={bound:.3e}")
    assert 0.0 < ref < 1.0 and abs(tr[0]["t"] - ref) <= bound, (tr[0]["t"], ref, bound)


def test_unbounded_lbfgs_commits_every_pair(qn):
    """lbfgs_cases.reject_fn (test_gpu_lbfgs.py's rejected-pair family): with BackTracking the second and third pairs have y = 0 and are dropped;
    with StrongWolfe the curvature condition makes every step leave the linear band's flat gradient behind: s.y > 0 in every iteration"""
    x0 = np.array(LC.REJECT_X0)
    w = LC.REJECT_WINDOW
    bt = qn.LBFGS(LC.TOL, x0, m=5)
    bt.set_trace(w)
    try:
        bt.minimize(qn.BackTracking(1e-4, 0.5), LC.reject_fn, w, 50)
    except qn.MaxIterReached:
        pass
    dropped = [r["updated"] for r in bt.trace()[0]]
    assert dropped[:3] == [1, 0, 0] == LC.ref_reject(5)[0].updated[:3]
    case = ("lbfgs", "reject", 3, 5, None)
    ref, rls, _, rstatus = W.ref_case(case)
    sw = qn.LBFGS(LC.TOL, x0, m=5)
    sw.set_trace(w, with_x=True)
    sw.minimize(qn.StrongWolfe(), LC.reject_fn, w, 50)  # converges inside the cap, as the restatement does
    tr, xs = sw.trace()
    assert rstatus == "ok" and len(tr) == len(ref.trace) >= 2
    assert [r["updated"] for r in tr] == [1] * len(tr) == ref.updated and sw.resets() == 0
    for k in range(len(tr)):
        if k < W.window(case):  # (behind it the restatement's own runs differ in a knife-edge decision: the iterates stay together, as below)
            assert tr[k]["ls_cases"] == rls.history[k]["ls_cases"] and tr[k]["ls_iters"] == ref.trace[k]["ls_iters"], k
        assert np.linalg.norm(xs[k] - ref.trace_x[k]) <= 1e-9 * max(1.0, np.linalg.norm(ref.trace_x[k])), k


def test_boxed_step_stops_on_the_face(qn):
    """t_max large, the face one trial away: f is linear along d, so the first trial (t = 1) asks for the largest extrapolation and the box cuts it to
    the face at t = 3; the search ends there (stp = stpmax).  No coordinate leaves the search's box, and the line-search value keeps its t_max."""
    lin = lambda p: (-float(p[0] + 0.5 * p[1]), np.array([-1.0, -0.5]))  # noqa: E731
    seen = []

    def fn(p):
        seen.append(p.copy())
        return lin(p)
    llb, lub = np.array([-1.0, -1.0]), np.array([3.0, 2.0])
    ls = qn.StrongWolfe().with_t_max(1e6).with_lower_bound(llb).with_upper_bound(lub)
    s = qn.ProjectedGradientDescent(0.0, [0.0, 0.0], [-np.inf, -np.inf], [np.inf, np.inf])
    s.set_trace(1, with_x=True)
    with pytest.raises(qn.MaxIterReached):
        s.minimize(ls, fn, 1, 20)
    tr, xs = s.trace()
    assert tr[0]["t"] == 3.0 and tr[0]["ls_iters"] == 2 and xs[0].tolist() == [3.0, 1.5]
    assert all(np.all(p >= llb) and np.all(p <= lub) for p in seen)
    assert ls.t_max() == 1e6 and ls.s.t_max == 1e6
    rl = RW.StrongWolfe(t_max=1e6, lower_bound=llb, upper_bound=lub)
    assert rl.compute_step_len(np.zeros(2), lin(np.zeros(2)), np.array([1.0, 0.5]), R.CountingOracle(lin), 20) == 3.0
    assert tr[0]["ls_cases"] == rl.history[0]["ls_cases"]


def _quartic(x):
    return float(np.sum(0.25 * x ** 4 - x)), x ** 3 - 1.0


def test_iteration_cap_of_the_search(qn):
    x0, lb, ub = np.array([0.0, -1.5]), np.full(2, -np.inf), np.full(2, np.inf)  # (t = 1 overshoots: f rises, the first trial does not end the search)
    for cap in (0, 1):
        calls = []

        def fn(p):
            calls.append(1)
            return _quartic(p)
        o = R.CountingOracle(_quartic)
        ref = R.ProjectedGradientDescent(0.0, x0, lb, ub)
        rl = RW.StrongWolfe(dot=RW.seq_dot)
        with pytest.raises(R.MaxIterReached):
            ref.minimize(rl, o, 2, cap)
        s = qn.ProjectedGradientDescent(0.0, x0, lb, ub)
        s.set_trace(2, with_x=True)
        with pytest.raises(qn.MaxIterReached):
            s.minimize(qn.StrongWolfe(), fn, 2, cap)
        tr, xs = s.trace()
        assert [r["t"] for r in tr] == [r["t"] for r in ref.trace] and [r["ls_iters"] for r in tr] == [cap, cap]
        assert xs.tobytes() == np.array(ref.trace_x).tobytes() and len(calls) == o.calls
        assert (tr[0]["t"] == 1.0) if cap == 0 else (0.0 < tr[0]["t"] < 1.0)  # the first trial / the next step, never evaluated by the search
        assert [h["evaluated"] for h in rl.history] == [False, False]


def test_non_finite_first_trial(qn):
    """a closure that returns inf beyond a radius: the first trial is outside, the bracket [0, 1] is bisected until a trial is finite"""
    def walled(p):
        return (np.inf, np.full(2, np.nan)) if float(p @ p) > 4.0 else _quartic(p)
    x0, g0 = np.array([0.0, 0.0]), np.array([-4.0, -4.0])  # (a start whose -g points far outside the wall)
    fn = lambda p: walled(p) if p.any() else (0.0, g0.copy())  # noqa: E731
    lb, ub = np.full(2, -np.inf), np.full(2, np.inf)
    ref = R.ProjectedGradientDescent(0.0, x0, lb, ub)
    rl = RW.StrongWolfe(dot=RW.seq_dot)
    with pytest.raises(R.MaxIterReached):
        ref.minimize(rl, R.CountingOracle(fn), 1, 20)
    assert rl.history[0]["cases"][:2] == [5, 5] and rl.history[0]["evaluated"]
    s = qn.ProjectedGradientDescent(0.0, x0, lb, ub)
    s.set_trace(1, with_x=True)
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.StrongWolfe(), fn, 1, 20)
    tr, xs = s.trace()
    assert tr[0]["t"] == ref.trace[0]["t"] and tr[0]["ls_cases"] == rl.history[0]["ls_cases"] and tr[0]["ls_iters"] == ref.trace[0]["ls_iters"]
    assert float(xs[0] @ xs[0]) <= 4.0 and np.isfinite(s.x()).all()


def test_not_a_descent_direction(qn):
    """g.d >= 0 at the start (dcsrch's input error): QN_ABNORMAL_TERMINATION, x stays at x_k.  A gradient that lies about its sign gives it."""
    x0 = np.array([1.0, 2.0, 3.0])
    s = qn.ProjectedGradientDescent(0.0, x0, np.full(3, -np.inf), np.full(3, np.inf))
    zero = lambda p: (1.0, np.array([0.0, 1e-300, 0.0]))  # noqa: E731 -- g.d = -1e-600 underflows to -0.0: not < 0
    with pytest.raises(qn.AbnormalTermination, match="not a descent direction"):
        s.minimize(qn.StrongWolfe(), zero, 5, 5)
    assert s.x().tolist() == x0.tolist() and s.k() == 0
    # ProjectedLBFGS with an active box can meet it: the restatement's boxed quadratic case stops the same way, at the same iteration
    case = ("lbfgs", "quad", 2050, 5, 0.05)
    ref, _, _, status = W.ref_case(case)
    assert status == "not_descent"
    q, b, _, _ = LC.quad_problem(2050)
    s2 = None
    with pytest.raises(qn.AbnormalTermination, match="not a descent direction"):
        lb, ub = W.box_of(2050, 0.05)
        s2 = qn.ProjectedLBFGS(W.TOL, W.problem("quad", 2050)[1], lb, ub, m=5)
        s2.set_trace(W.ITERS, with_x=True)
        s2.minimize(_ls(qn, case), qn.Quadratic(q, b), W.ITERS, W.MAX_LS)
    assert s2.k() == len(ref.trace)
    assert np.linalg.norm(s2.x() - ref.x) <= 1e-9 * max(1.0, np.linalg.norm(ref.x))


def test_determinism_syncs_warm_restart_callbacks_and_path(qn):
    case = ("lbfgs", "lse", 2050, 17, None)
    w = W.window(case)
    o = _Oracle(qn, case)
    ks = []
    x0 = W.problem("lse", 2050)[1]
    lb, ub = W.box_of(2050, None)
    one = qn.ProjectedLBFGS(W.TOL, x0, lb, ub, m=17)
    one.set_trace(w, with_x=True)
    before = one.stats()["host_syncs"]
    with pytest.raises(qn.MaxIterReached):
        one.minimize(_ls(qn, case), o.o, w, W.MAX_LS, lambda r: ks.append(r.k()))
    two, _, _ = _gpu(qn, case, o.o, w)
    assert one.trace()[1].tobytes() == two.trace()[1].tobytes() and ks == list(range(1, w + 1))
    st = one.stats()
    st["host_syncs"] -= before
    tr, _ = one.trace()
    extra = sum(r["ls_iters"] - 1 for r in tr)
    assert st["host_syncs"] <= w + extra + 2, (st["host_syncs"], w, extra)  # one per iteration, one per further trial, a constant
    assert st["path"] == PATH_VECTOR | PATH_LBFGS and st["iterations"] == w
    # the same run in two calls: the memory, the memo and dcsrch's state (none survives a search) carry over bit for bit
    half = w // 2
    s = qn.ProjectedLBFGS(W.TOL, x0, lb, ub, m=17)
    ls = _ls(qn, case)
    for iters in (half, w - half):
        with pytest.raises(qn.MaxIterReached):
            s.minimize(ls, o.o, iters, W.MAX_LS)
    assert s.x().tobytes() == one.x().tobytes()
    # a host closure is called only for points the machine asked for: the restatement's sequence
    case = ("lbfgs", "host", 7, 1, None)
    w = W.window(case)
    _, _, ro, _ = W.run_ref(case, iters=w)
    calls = []
    fn = W.problem("host", 7)[0]

    def counted(p):
        calls.append(1)
        return fn(p)
    h, _, _ = _gpu(qn, case, counted, w, memoize=0)
    assert len(calls) == ro.calls == h.stats()["oracle_calls"]


def test_rejections(qn):
    q, b, x0, _ = LC.quad_problem(7)
    obj = qn.Quadratic(q, b)
    h = np.eye(7)
    for s in (qn.BFGS(1e-8, x0), qn.Newton(1e-8, x0), qn.GradientDescent(1e-8, x0), qn.Broyden(1e-8, x0)):
        with pytest.raises(qn.ErrorInputParams):
            s.minimize(qn.StrongWolfe(), obj if not isinstance(s, qn.Newton) else (lambda p: (0.5 * float(p @ p), p, h)), 5, 5)
    lb, ub = LC.free_box(7)
    for bad in ((0.0, 0.9), (0.5, 0.4), (1e-4, 1.0), (-1.0, 0.5), (0.3, 0.3)):
        with pytest.raises(qn.ErrorInputParams, match="c1"):
            qn.LBFGS(1e-8, x0).minimize(qn.StrongWolfe(*bad), obj, 5, 5)
    with pytest.raises(qn.ErrorInputParams):
        qn.StrongWolfe().with_xtol(-1.0)
    with pytest.raises(qn.ErrorInputParams):
        qn.LBFGS(1e-8, x0).minimize(qn.StrongWolfe().with_t_min(2.0).with_t_max(1.0), obj, 5, 5)
    with pytest.raises(qn.ErrorInputParams):
        qn.StrongWolfe().compute_step_len(x0, (1.0, np.ones(7)), -np.ones(7), lambda p: (float(p @ p), 2 * p), 5)
    # More-Thuente on these solvers: today's error, today's text
    with pytest.raises(qn.ErrorInputParams, match="More-Thuente"):
        qn.SpectralProjectedGradient(1e-8, x0, obj, lb, ub).minimize(qn.MoreThuente(), obj, 5, 5)
    with pytest.raises(qn.ErrorInputParams, match="More-Thuente"):
        qn.LBFGS(1e-8, x0).minimize(qn.MoreThuente(), obj, 5, 5)
    ls = qn.StrongWolfe(1e-3, 0.5).with_xtol(0.2).with_t_min(0.1).with_t_max(50.0)
    assert (ls.s.kind, ls.s.c1, ls.s.c2, ls.s.delta, ls.s.t_min, ls.s.t_max) == (6, 1e-3, 0.5, 0.2, 0.1, 50.0)
    d = qn.StrongWolfe()
    assert (d.s.c1, d.s.c2, d.xtol(), d.t_min(), d.t_max()) == (1e-4, 0.9, 0.1, 0.0, 1e10)
