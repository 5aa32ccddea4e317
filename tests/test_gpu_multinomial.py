"""GPU tests of the device multinomial objective (qn.Multinomial; kernel csrc/qn_multinomial.hip.h, the combines csrc/qn_logistic.hip.h and
csrc/qn_lse_hv.hip.h): the evaluation, P and the Hessian-vector product against np.longdouble inside the derived bounds of tests/ref_multinomial.py
(C = 8 is a cap, not a measurement), saturation, K = 2 against the existing Logistic, bit-for-bit repeatability, the refusals, NewtonCG against the
restatement inside the windows tests/test_ref_multinomial.py licenses, and the rest of the O(n) family against the existing restatements run on
ref_multinomial.multinomial_fn and beside a host closure of it.  The largest |error| / bound per quantity is printed, and recorded in README."""
import numpy as np
import pytest

import multinomial_cases as MC
import ref_logistic as RL
import ref_multinomial as RM
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
LD = np.longdouble
_worst = {}


def _obj(qn, pr, mu=None, ctx=None, kernel=1):
    """the objective with the register-blocked kernel streaming A at every K (the automatic choice above 16 classes is the MFMA kernel, which
    tests/test_gpu_multinomial_mfma.py holds to the same checks)"""
    a, y, w, k, mu0 = pr[:5]
    obj = qn.Multinomial(a, y, k, mu0 if mu is None else mu, weights=w, ctx=ctx)
    obj.set_kernel(kernel)
    return obj


def _note(ratios):
    for k, r in ratios.items():
        _worst[k] = max(_worst.get(k, 0.0), r)


def _check_point(obj, pr, x, truth, tag, product=True):
    ev = obj(x)
    got = dict(f=ev.f(), g=ev.g(), p=obj.probabilities(x))
    if product:
        got["q"], got["c"] = obj.hess_vec_at(x, pr[6])
    r = RM.ratios(got, truth)
    _note(r)
    print(f"multinomial {tag}: |error| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (tag, r)
    return got


# ---- 1. the evaluation, P and the product inside the bounds ----
@pytest.mark.parametrize("m,n,k", MC.SHAPES)
def test_everything_inside_the_bounds(qn, m, n, k):
    """f, g, P, H v and v'Hv against longdouble at x = 1e-3 / 1 / 30 times x0 on the weighted problem (masked rows wherever the draw put them), and at
    x0 with unit weights, with the first and the last row of a workgroup's cut masked, and with a class that no row carries"""
    for kind, scales in (("weighted", MC.SCALES), ("unit", [1.0]), ("edges", [1.0]), ("absent", [1.0])):
        obj = None
        try:
            for scale in scales:
                pr, x, truth = MC.truth_at(m, n, k, scale, kind)
                obj = obj or _obj(qn, pr)
                got = _check_point(obj, pr, x, truth, f"{(m, n, k)} {kind} scale {scale:g}")
                # v'Hv matches the returned vector: the shares' sum of v_j q_j, N products in another order
                v = pr[6]
                vq = np.sum(v.astype(LD) * got["q"].astype(LD))
                assert abs(LD(got["c"]) - vq) <= LD(RM.gamma(k * n + 2)) * np.sum(np.abs(v * got["q"]).astype(LD))
        finally:
            if obj:
                obj.close()
    print("multinomial worst |error| / bound so far:", {k: f"{v:.3f}" for k, v in _worst.items()})


@pytest.mark.parametrize("m,n,k", MC.CUT_SHAPES + MC.LDS_SHAPES)
def test_every_instance_and_cut(qn, m, n, k):
    """the instances of the kernel and the cuts of its threads that the shapes above do not select (multinomial_cases.CUT_SHAPES), and the shapes whose
    row tiles are cut down to fit LDS beside W (multinomial_cases.LDS_SHAPES), at x0"""
    pr, x, truth = MC.truth_at(m, n, k, 1.0)
    obj = _obj(qn, pr)
    try:
        _check_point(obj, pr, x, truth, f"{(m, n, k)} cut")
    finally:
        obj.close()


@pytest.mark.parametrize("m,n,k", [(17, 7, 3), (1031, 12, 4)])
def test_a_masked_row_whose_margins_overflow(qn, m, n, k):
    """the masked row holds +-1e300 and the point +-1e10 in its first columns: its margins are +-inf, their differences NaN; f, g, P, H v are those of the
    problem with the row deleted -- the same bits where the cut of the remaining rows is the same, inside the bounds either way -- and nothing is NaN"""
    pr = MC.variant(m, n, k, "overflow")
    x = MC.overflow_point(pr)
    a, y, w = pr[0], pr[1], pr[2]
    tame = a.copy()
    tame[m // 2, :] = 0.0  # the same row cut, the masked row harmless: the bits must not change
    obj, ref = _obj(qn, pr), qn.Multinomial(tame, y, k, pr[4], weights=w)
    try:
        ev, ev2 = obj(x), ref(x)
        q, c = obj.hess_vec_at(x, pr[6])
        q2, c2 = ref.hess_vec_at(x, pr[6])
        p = obj.probabilities(x)
        assert np.isfinite(ev.f()) and np.all(np.isfinite(ev.g())) and np.all(np.isfinite(q)) and np.isfinite(c) and np.all(np.isfinite(p))
        assert ev.f() == ev2.f() and ev.g().tobytes() == ev2.g().tobytes() and q.tobytes() == q2.tobytes() and c == c2
        assert np.all(p[m // 2] == 0.0)
    finally:
        obj.close()
        ref.close()


def test_saturated_margins(qn):
    """margins spread by 1600: the loss of the row labelled with the loser equals the spread, the losers' p are exactly 0.0, nothing is NaN"""
    a, y, w, k, mu, x, spread = MC.saturated_problem()
    truth = RM.truth_and_bound(a, y, w, k, mu, x, np.ones(x.size))
    obj = qn.Multinomial(a, y, k, mu, weights=w)
    zero = qn.Multinomial(a[:1], y[:1], k, 0.0)
    try:
        _check_point(obj, (a, y, w, k, mu, None, np.ones(x.size)), x, truth, "saturated")
        p = obj.probabilities(x)
        assert p[0, 0] == 1.0 and p[0, 1] == 0.0 and p[0, 2] == 0.0 and np.all(p[2] == 0.0) and not np.any(np.isnan(p))
        ev = zero(x)
        assert ev.f() == spread and not np.any(np.isnan(ev.g()))  # (row 0 alone, mu = 0: the loss IS the spread)
        assert ev.g()[0] == 1.0 and ev.g()[2] == -1.0 and ev.g()[4] == 0.0  # (p_0 - 0) a, (p_1 - 1) a, (p_2 - 0) a in the first column
    finally:
        obj.close()
        zero.close()


def test_k_2_is_the_logistic_objective(qn):
    """with mu = 0 on both, f(W) = f_logistic(W_1 - W_0), g_1 = -g_0 = g_logistic within the sum of the two objects' bounds, and sum_k g_k = 0"""
    for (m, n) in [(17, 8), (257, 40)]:
        a, y, w, k, _, x0, v = MC.problem(m, n, 2)
        ys = 2.0 * y - 1.0
        mn, lg = qn.Multinomial(a, y, 2, 0.0, weights=w), qn.Logistic(a, ys, 0.0, weights=w)
        try:
            xd = x0[n:] - x0[:n]
            tm = RM.truth_and_bound(a, y, w, 2, 0.0, x0)
            tl = RL.truth_and_bound(a, ys, w, 0.0, xd)
            em, el = mn(x0), lg(xd)
            # (W_1 - W_0 is formed in float64 by the test: its rounding moves the logistic point by at most dz per margin)
            dz = LD(RL.gamma(2)) * (np.abs(a).astype(LD) @ (np.abs(x0[n:]) + np.abs(x0[:n])).astype(LD))  # |a_r . (xd - (W_1 - W_0))|
            bshift_f = np.sum(w.astype(LD) * dz)
            bshift_g = np.abs(a).astype(LD).T @ (w.astype(LD) * dz / 4)
            assert abs(LD(em.f()) - LD(el.f())) <= tm["bf"] + tl["bf"] + bshift_f
            g = em.g().astype(LD)
            assert np.all(np.abs(g[n:] - el.g().astype(LD)) <= tm["bg"][n:] + tl["bg"] + bshift_g)
            assert np.all(np.abs(g[:n] + el.g().astype(LD)) <= tm["bg"][:n] + tl["bg"] + bshift_g)
            assert np.all(np.abs(g[:n] + g[n:]) <= tm["bg"][:n] + tm["bg"][n:])
        finally:
            mn.close()
            lg.close()


def test_same_bits_from_call_to_call_and_object_to_object(qn):
    for (m, n, k) in [(64, 41, 17), (1031, 12, 4), (20, 1024, 16)]:
        pr, x, _ = MC.truth_at(m, n, k, 1.0)
        one, two = _obj(qn, pr), qn.Multinomial(pr[0].copy(), pr[1].copy(), k, pr[4], weights=pr[2].copy())
        try:
            two.set_kernel(1)
            a1, a2, b1 = one(x), one(x), two(x)
            assert a1.f() == a2.f() == b1.f() and a1.g().tobytes() == a2.g().tobytes() == b1.g().tobytes()
            (q1, c1), (q2, c2), (q3, c3) = one.hess_vec_at(x, pr[6]), one.hess_vec_at(x, pr[6]), two.hess_vec_at(x, pr[6])
            assert q1.tobytes() == q2.tobytes() == q3.tobytes() and c1 == c2 == c3
            one(30.0 * x)  # an evaluation elsewhere does not move the product at x (hess_vec_at forms P at x itself)
            q4, c4 = one.hess_vec_at(x, pr[6])
            assert q4.tobytes() == q1.tobytes() and c4 == c1
            assert one.probabilities(x).tobytes() == two.probabilities(x).tobytes()
        finally:
            one.close()
            two.close()


# ---- 2. refusals: each ErrorInputParams with its message, before anything is launched ----
def test_creation_refusals(qn):
    rng = np.random.default_rng(5)
    a, y = rng.standard_normal((4, 3)), np.array([0, 2, 1, 0])
    for bad in (3, -1, 1.5):
        yb = y.astype(np.float64)
        yb[2] = bad
        with pytest.raises(qn.ErrorInputParams, match=r"labels\[2\]"):
            qn.Multinomial(a, yb, 3, 0.5)
    for bad in (-1.0, float("nan"), float("inf")):
        w = np.ones(4)
        w[1] = bad
        with pytest.raises(qn.ErrorInputParams, match=r"weights\[1\] is negative or not finite"):
            qn.Multinomial(a, y, 3, 0.5, weights=w)
    with pytest.raises(qn.ErrorInputParams, match="mu must be finite"):
        qn.Multinomial(a, y, 3, float("nan"))
    with pytest.raises(qn.ErrorInputParams, match="fewer than 2 classes"):
        qn.Multinomial(a, np.zeros(4), 1, 0.5)
    with pytest.raises(qn.ErrorInputParams, match="not built for a padded K n > 16384"):
        qn.Multinomial(np.zeros((2, 1025)), np.array([0, 1]), 16, 0.5)  # (N_pad = 16400: one tile past)
    with pytest.raises(qn.ErrorInputParams, match="not built for more than 256 classes"):
        qn.Multinomial(np.zeros((2, 2)), np.array([0, 1]), 257, 0.5)
    ok = qn.Multinomial(a, y, 4, -3.0)  # (any finite mu; class 3 is carried by no row)
    assert ok.n == 12 and ok.n_classes == 4
    ok.close()


def test_a_two_rank_context_is_refused(qn):
    def gather(send, recv):
        recv[:send.size] = send
        recv[send.size:] = send
    ctx = qn.Context(0, 0, 2, host_allgather=gather)  # (world = 2 through the host exchange, this rank alone)
    try:
        with pytest.raises(qn.ErrorInputParams, match="single-GPU"):
            qn.Multinomial(np.ones((4, 3)), np.array([0, 1, 2, 0]), 3, 0.5, ctx=ctx)
    finally:
        ctx.close()


def test_solver_and_entry_point_refusals(qn):
    pr = MC.problem(3, 1, 5)
    obj = _obj(qn, pr)
    quad = qn.Quadratic(np.eye(5), np.zeros(5))
    x0 = pr[5]
    try:
        lb, ub = np.full(5, -1.0), np.full(5, 1.0)
        refused = [(qn.BFGS(1e-8, x0), "Multinomial"), (qn.DFP(1e-8, x0), "Multinomial"), (qn.Broyden(1e-8, x0), "Multinomial"),
                   (qn.GradientDescent(1e-8, x0), "Multinomial"), (qn.CoordinateDescent(1e-8, x0), "Multinomial"), (qn.Newton(1e-8, x0), "Multinomial"),
                   (qn.ProjectedNewton(1e-8, x0, lb, ub), "Hessian not available")]
        for solver, message in refused:
            try:
                with pytest.raises(qn.ErrorInputParams, match=message):
                    solver.minimize(qn.BackTracking(1e-4, 0.5), obj, 5, 5)
                assert solver.stats()["launches"] == 0, type(solver).__name__
            finally:
                solver.close()
        with pytest.raises(qn.ErrorInputParams, match="Hessian not available"):
            qn.SpectralProjectedNewton(1e-8, x0, obj, lb, ub)
        spn = qn.SpectralProjectedNewton(1e-8, x0, lambda p: (0.5 * float(p @ p), p, np.eye(5)), lb, ub)
        try:
            before = spn.stats()["launches"]
            with pytest.raises(qn.ErrorInputParams, match="Hessian not available"):
                spn.minimize(qn.BackTracking(1e-4, 0.5), obj, 5, 5)
            assert spn.stats()["launches"] == before
        finally:
            spn.close()
        s = qn.LBFGS(1e-8, x0)
        with pytest.raises(qn.ErrorInputParams, match="needs a device quadratic"):
            s.minimize(qn.ExactQuadratic(), obj, 5, 5)
        assert s.stats()["launches"] == 0
        s.close()
        with pytest.raises(qn.ErrorInputParams, match="dense Hessian of a multinomial objective"):
            obj.hessian(x0)
        with pytest.raises(qn.ErrorInputParams, match="hess_vec_at"):
            obj.hess_vec(x0)
        with pytest.raises(qn.ErrorInputParams, match="get_rows is not built for a multinomial"):
            obj.rows(0, 1)
        n1, n2, n3, n4 = (qn._abi.C.c_size_t(), qn._abi.C.c_int(), qn._abi.C.c_size_t(), qn._abi.C.c_int())
        C = qn._abi.C
        assert qn._abi.lib().qn_objective_sparse_info(obj.h, C.byref(n1), C.byref(n2), C.byref(n3), C.byref(n4)) != 0
        tn = qn.NewtonCG(1e-7, x0)
        with pytest.raises(qn.ErrorInputParams, match="BackTracking or StrongWolfe"):
            tn.minimize(qn.GLLQuadratic(1e-4, 10), obj, 5, 5)
        assert tn.stats()["launches"] == 0
        tn.close()
    finally:
        obj.close()
        quad.close()


# ---- 3. NewtonCG against the restatement, inside the licensed windows ----
def _ls(qn, kind):
    return qn.StrongWolfe(*MC.WOLFE) if kind == "wolfe" else qn.BackTracking(1e-4, 0.5)


def newton_run(qn, m, n, k, ls, iters=MC.ITERS, memoize=1, chunk=8, mu=None, calls=1, kernel=1):
    pr = MC.problem(m, n, k)
    obj = _obj(qn, pr, mu, kernel=kernel)
    s = qn.NewtonCG(MC.TOL, pr[5], chunk=chunk, memoize=memoize)
    out = dict(trace=[], xs=[], inner=[], neg=[], fb=[], hv=0, inner_total=0, status="ok", k=0)
    try:
        for _ in range(calls):
            s.set_trace(iters, with_x=True)
            rec = []
            try:
                s.minimize(_ls(qn, ls), obj, iters, MC.MAX_LS, callback=lambda sv: rec.append((sv.inner_iterations()[0], sv.negative_curvature(), sv.fallbacks())))
                out["status"] = "ok"
            except qn.MaxIterReached:
                out["status"] = "max_iter"
            tr, xs = s.trace()
            st = s.stats()
            out["trace"] += list(tr)
            out["xs"] += [np.array(x) for x in xs]
            out["inner"] += [r[0] for r in rec]
            out["neg"] += [r[1] for r in rec]
            out["fb"] += [r[2] for r in rec]
            out["hv"] += s.hv_passes()
            out["inner_total"] += s.inner_iterations()[1]
            out["k"] += s.k()
            out["obj_bytes"], out["evals"], out["launches"], out["path"] = st["obj_bytes"], st["oracle_evals"], st["launches"], st["path"]
        out["x"] = s.x()
    finally:
        s.close()
        obj.close()
    return out


def _bits(run):
    return (run["x"].tobytes(), [x.tobytes() for x in run["xs"]], [(r["t"], r["n_evals"], r["f"]) for r in run["trace"]], run["inner"], run["status"])


_runs = {}


def _run(qn, m, n, k, ls, memoize):
    key = (m, n, k, ls, memoize)
    if key not in _runs:
        _runs[key] = newton_run(qn, m, n, k, ls, memoize=memoize)
    return _runs[key]


@pytest.mark.parametrize("m,n,k,ls", MC.CASES)
def test_newton_cg_against_the_restatement(qn, m, n, k, ls):
    w = MC.window(m, n, k, ls)
    ref, _, ref_status = MC.ref_case(m, n, k, ls)
    run = _run(qn, m, n, k, ls, 1)
    assert len(run["trace"]) >= w and len(run["inner"]) == len(run["trace"])
    worst = 0.0
    for i in range(w):
        r, g = ref.trace[i], run["trace"][i]
        dx = float(np.linalg.norm(run["xs"][i] - ref.trace_x[i]) / max(1.0, np.linalg.norm(ref.trace_x[i])))
        worst = max(worst, dx)
        assert dx <= MC.GPU_TOL, (i, dx)
        assert g["n_evals"] == r["n_evals"] and g["ls_iters"] == r["ls_iters"], (i, g, r)
        assert (g["t"] == r["t"]) if ls == "bt" else (abs(g["t"] - r["t"]) <= MC.GPU_TOL * abs(r["t"])), (i, g["t"], r["t"])
        assert run["inner"][i] == ref.inner[i], (i, run["inner"], ref.inner)
    assert run["neg"][w - 1] == 0 and run["fb"][w - 1] == 0
    # every shape converges to 1e-7 in the restatement's iteration count, under both searches
    assert run["status"] == "ok" and ref_status == "ok" and run["k"] == ref.k, (run["k"], ref.k, run["status"])
    pr = MC.problem(m, n, k)
    g = RM.truth_and_bound(pr[0], pr[1], pr[2], k, pr[4], run["x"])["g"]
    assert float(np.max(np.abs(g))) < MC.TOL
    assert run["hv"] == run["inner_total"] == sum(run["inner"])
    assert run["path"] & qn._abi.PATH_NEWTON_CG and run["path"] & qn._abi.PATH_VECTOR
    print(f"multinomial NewtonCG {(m, n, k, ls)}: window {w} of {len(ref.trace)}, worst |x - x_ref| = {worst:.2e}, GPU k = {run['k']} ({run['status']})")


@pytest.mark.parametrize("m,n,k,ls", [(96, 16, 4, "bt"), (64, 41, 17, "wolfe")])
def test_memoize_0_and_1_give_the_same_bits(qn, m, n, k, ls):
    assert _bits(_run(qn, m, n, k, ls, 0)) == _bits(_run(qn, m, n, k, ls, 1))


def test_launch_and_byte_accounting(qn):
    m, n, k = 96, 16, 4
    run = _run(qn, m, n, k, "bt", 1)
    g_wg = MC.row_cut(m)[0]
    one = 8 * (m * (16 * ((n + 15) // 16) + k) + g_wg * 16 * ((k * n + 15) // 16))
    # evaluations + products + ONE weights pass per loop top (k outer iterations and the loop top that found the run converged)
    assert run["obj_bytes"] == (run["evals"] + run["hv"] + run["k"] + 1) * one, (run["obj_bytes"], run["evals"], run["hv"], run["k"])


def test_negative_mu_takes_the_gradient(qn):
    ghg, gg = MC.neg_mu_curvature()
    assert ghg < 0.0 < gg  # chosen on the host: rule 4 at j = 0
    m, n, k = MC.NEG_SHAPE
    ref = MC.run_ref(m, n, k, "bt", iters=3, mu=MC.NEG_MU)[0]
    assert ref.why[0] == "negcurv" and ref.inner[0] == 0
    run = newton_run(qn, m, n, k, "bt", iters=3, mu=MC.NEG_MU)
    assert run["neg"][0] >= 1 and run["inner"][0] == 0
    pr = MC.problem(m, n, k)
    g0 = RM.multinomial_fn(pr[0], pr[1], pr[2], k, MC.NEG_MU)(pr[5])[1]
    t0 = run["trace"][0]["t"]
    assert np.linalg.norm(run["xs"][0] - (pr[5] + t0 * -g0)) <= MC.GPU_TOL * max(1.0, np.linalg.norm(pr[5]))  # d = -g


def test_two_calls_are_one(qn):
    one = newton_run(qn, 96, 16, 4, "bt", iters=8)
    two = newton_run(qn, 96, 16, 4, "bt", iters=4, calls=2)
    assert one["x"].tobytes() == two["x"].tobytes() and one["inner"] == two["inner"]
    assert [x.tobytes() for x in one["xs"]] == [x.tobytes() for x in two["xs"]]


# ---- 4. the rest of the family: the existing restatements on multinomial_fn, and beside a host closure of it ----
def _family_gpu(qn, kind, m, n, k, oracle, iters, memoize=1):
    pr = MC.problem(m, n, k)
    lb, ub = MC.family_box(kind, k * n)
    if kind == "lbfgs":
        s, ls = qn.LBFGS(MC.FAMILY_TOL, pr[5], m=5, memoize=memoize), qn.StrongWolfe()
    elif kind == "cg":
        s, ls = qn.NonlinearCG(MC.FAMILY_TOL, pr[5], variant="pr+", memoize=memoize), qn.StrongWolfe(1e-4, 0.1)
    elif kind == "spg":
        s, ls = qn.SpectralProjectedGradient(MC.FAMILY_TOL, pr[5], oracle, lb, ub, memoize=memoize), qn.GLLQuadratic(1e-4, 10)
    else:
        s, ls = qn.ProjectedLBFGS(MC.FAMILY_TOL, pr[5], lb, ub, m=5, memoize=memoize), qn.BackTrackingB(1e-4, 0.5, lb, ub)
    s.set_trace(iters, with_x=True)
    try:
        s.minimize(ls, oracle, iters, 50)
    except qn.MaxIterReached:
        pass
    return s


@pytest.mark.parametrize("kind,m,n,k", MC.FAMILY_CASES)
def test_the_rest_of_the_family(qn, kind, m, n, k):
    ref, w = MC.family_licence(kind, m, n, k)
    assert w >= 4
    pr = MC.problem(m, n, k)
    fn = RM.multinomial_fn(pr[0], pr[1], pr[2], k, pr[4])
    obj = _obj(qn, pr)
    dev = host = dev0 = None
    try:
        dev = _family_gpu(qn, kind, m, n, k, obj, w)
        dev0 = _family_gpu(qn, kind, m, n, k, obj, w, memoize=0)
        host = _family_gpu(qn, kind, m, n, k, lambda x: fn(x), w)
        ref_w = type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
        for run in (dev, host):
            _compare(run, ref_w, w)
            if kind != "spg":
                tr = run.trace()[0]
                assert [r["updated"] for r in tr[:w]] == ref.updated[:w]
        (dt, dx), (ht, hx) = dev.trace(), host.trace()
        for i in range(w):  # the device objective beside the host closure: equal decisions, x within the family's tolerance
            assert dt[i]["n_evals"] == ht[i]["n_evals"] and dt[i]["ls_iters"] == ht[i]["ls_iters"], i
            assert np.linalg.norm(dx[i] - hx[i]) <= 1e-9 * max(1.0, np.linalg.norm(hx[i])), i
        assert dev0.x().tobytes() == dev.x().tobytes() and [x.tobytes() for x in dev0.trace()[1]] == [x.tobytes() for x in dx]  # memoize 0 / 1: the same bits
        sd, sh = dev.stats(), host.stats()
        extra = sd["launches"] - sh["launches"]  # TWO launches per evaluation (the batch whose loop top ends the run may enqueue one nobody asked for)
        print(f"multinomial {kind} {(m, n, k)}: window {w}, launches device {sd['launches']} host {sh['launches']}, evaluations {sd['oracle_evals']}")
        assert extra % 2 == 0 and extra // 2 - sd["oracle_evals"] in (0, 1), (extra, sd["oracle_evals"])
    finally:
        for run in (dev, host, dev0):
            if run is not None:
                run.close()
        obj.close()
