"""GPU tests of the device logistic objective (qn.Logistic; kernels csrc/qn_logistic.hip.h, the product's csrc/qn_lse_hv.hip.h): the evaluation and the
Hessian-vector product against np.longdouble inside the derived bounds of tests/ref_logistic.py (C = 8 is a cap, not a measurement), bit-for-bit
repeatability, NewtonCG against the restatement inside the windows tests/test_ref_logistic.py licenses, the rest of the O(n) family against the existing
restatements run on ref_logistic.logistic_fn and beside a host closure of it, and the refusals.

MEASURED on one MI355X (the largest |error| / bound over all shapes, scales and weightings, printed by the tests): f 0.181, g 0.145,
H v 0.062, v'Hv 0.073."""
import numpy as np
import pytest

import logistic_cases as LC
import ref_logistic as RL
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
LD = np.longdouble
_worst = {}


def _obj(qn, pr, mu=None, ctx=None):
    a, y, w, mu0, _, _ = pr
    return qn.Logistic(a, y, mu0 if mu is None else mu, weights=w, ctx=ctx)


def _note(key, ratios):
    for k, r in ratios.items():
        _worst[(key, k)] = max(_worst.get((key, k), 0.0), r)


# ---- 1. the evaluation ----
@pytest.mark.parametrize("m,n", LC.SHAPES)
def test_evaluation_inside_the_bounds(qn, m, n):
    """f and g against longdouble at the scales 1e-3, 1, 30: weighted problems (masked rows wherever the draw put them; (1, 1) and (3, 5) have fewer rows
    than workgroups), and at scale 1 the unit weights and the problem with the first and the last row of a workgroup's cut masked."""
    for kind, scales in (("weighted", LC.SCALES), ("unit", [1.0]), ("edges", [1.0])):
        obj = None
        try:
            for scale in scales:
                pr, x, truth = LC.truth_at(m, n, scale, kind)
                obj = obj or _obj(qn, pr)
                ev = obj(x)
                r = RL.ratios(dict(f=ev.f(), g=ev.g()), truth)
                _note("eval", r)
                print(f"logistic eval {(m, n)} {kind} scale {scale:g}: |f - f*| / bound = {r['f']:.3f}, max |g - g*| / bound = {r['g']:.3f}")
                assert r["f"] <= 1.0 and r["g"] <= 1.0, (kind, scale, r)
        finally:
            if obj:
                obj.close()
    print("logistic eval worst so far:", {k[1]: f"{v:.3f}" for k, v in _worst.items() if k[0] == "eval"})


def test_saturated_margins(qn):
    """margins of -800, +800, +800 (masked) and 0.5: f is finite and inside its bound (the loss of the first row is 800), s and d are exactly 0 on
    the saturated side -- g_1 is mu x_1 exactly, and the product sees no curvature from rows 0, 1 and 2"""
    a, y, w, mu, x, _ = LC.saturated_problem()
    truth = RL.truth_and_bound(a, y, w, mu, x)
    obj = qn.Logistic(a, y, mu, weights=w)
    try:
        ev = obj(x)
        r = RL.ratios(dict(f=ev.f(), g=ev.g()), truth)
        assert np.isfinite(ev.f()) and ev.f() > 800.0 and r["f"] <= 1.0 and r["g"] <= 1.0, (ev.f(), r)
        assert ev.g()[1] == mu * x[1]
        for j in range(3):
            e = np.zeros(3)
            e[j] = 1.0
            q, c = obj.hess_vec_at(x, e)
            d_j = float(truth["d"][3]) * 0.25 if j == 2 else 0.0  # (row 3 alone has curvature: d_3 a_3j^2)
            assert np.array_equal(q[:2], mu * e[:2]) and abs(q[2] - (d_j + mu * e[2])) <= 1e-15 and c == q[j], (j, q, c)
    finally:
        obj.close()


def test_same_bits_from_call_to_call_and_object_to_object(qn):
    for (m, n) in [(257, 200), (5, 4099), (1024, 1024)]:
        pr, x, _ = LC.truth_at(m, n, 1.0)
        one, two = _obj(qn, pr), qn.Logistic(pr[0].copy(), pr[1].copy(), pr[3], weights=pr[2].copy())
        try:
            a1, a2, b1 = one(x), one(x), two(x)
            assert a1.f() == a2.f() == b1.f() and a1.g().tobytes() == a2.g().tobytes() == b1.g().tobytes()
        finally:
            one.close()
            two.close()


def test_rows_come_back(qn):
    pr = LC.problem(40, 65)
    obj = _obj(qn, pr)
    try:
        assert np.array_equal(obj.rows(3, 5), pr[0][3:8]) and obj.m == 40 and obj.n == 65
    finally:
        obj.close()


# ---- 2. the Hessian-vector product ----
@pytest.mark.parametrize("m,n", LC.SHAPES)
def test_product_inside_its_bound(qn, m, n):
    """H(x) v and v'Hv against longdouble at the scales 1 and 30; a second product at the same x is bit-identical; a product after an evaluation at
    another point is still the product at x.  That last check guards the public call's contract only: `hess_vec_at` forms the weights at x itself before
    every product, so it cannot see an evaluation that wrote its d into the accepted point's buffer (`lw`) where it should write the trial buffer --
    nor can a NewtonCG run, which forms the weights afresh for every direction.  No entry point reads `lw` back."""
    for kind in ("weighted", "edges"):
        pr, x, truth = LC.truth_at(m, n, 1.0, kind)
        v = pr[5]
        obj = _obj(qn, pr)
        try:
            q, c = obj.hess_vec_at(x, v)
            r = RL.ratios(dict(q=q, c=c), truth)
            _note("product", r)
            print(f"logistic product {(m, n)} {kind}: max |q - q*| / bound = {r['q']:.3f}, |c - c*| / bound = {r['c']:.3f}")
            assert r["q"] <= 1.0 and r["c"] <= 1.0, (kind, r)
            # v'Hv matches the returned vector: the shares' sum of v_j q_j, n products in another order
            vq = np.sum(v.astype(LD) * q.astype(LD))
            assert abs(LD(c) - vq) <= LD(RL.gamma(n + 2)) * np.sum(np.abs(v * q).astype(LD))
            q2, c2 = obj.hess_vec_at(x, v)
            assert q2.tobytes() == q.tobytes() and c2 == c
            none, c3 = obj.hess_vec_at(x, v, download=False)
            assert none is None and c3 == c
            obj(30.0 * x)  # an evaluation elsewhere (see the docstring for what this does and does not show)
            q4, c4 = obj.hess_vec_at(x, v)
            assert q4.tobytes() == q.tobytes() and c4 == c
        finally:
            obj.close()
    pr, x, truth = LC.truth_at(m, n, 30.0)
    obj = _obj(qn, pr)
    try:
        q, c = obj.hess_vec_at(x, pr[5])
        r = RL.ratios(dict(q=q, c=c), truth)
        _note("product", r)
        assert r["q"] <= 1.0 and r["c"] <= 1.0, r
    finally:
        obj.close()
    print("logistic product worst so far:", {k[1]: f"{v:.3f}" for k, v in _worst.items() if k[0] == "product"})


# ---- 3. NewtonCG against the restatement, inside the licensed windows ----
def _ls(qn, kind):
    return qn.StrongWolfe(*LC.WOLFE) if kind == "wolfe" else qn.BackTracking(1e-4, 0.5)


def newton_run(qn, m, n, ls, iters=LC.ITERS, memoize=1, chunk=8, mu=None, calls=1):
    pr = LC.problem(m, n)
    obj = _obj(qn, pr, mu)
    s = qn.NewtonCG(LC.TOL, pr[4], chunk=chunk, memoize=memoize)
    out = dict(trace=[], xs=[], inner=[], neg=[], fb=[], hv=0, inner_total=0, status="ok", k=0, obj_bytes=0, evals=0, launches=0, np=0)
    try:
        for _ in range(calls):
            s.set_trace(iters, with_x=True)
            rec = []
            try:
                s.minimize(_ls(qn, ls), obj, iters, LC.MAX_LS, callback=lambda sv: rec.append((sv.inner_iterations()[0], sv.negative_curvature(), sv.fallbacks())))
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


def _run(qn, m, n, ls, memoize, chunk):
    key = (m, n, ls, memoize, chunk)
    if key not in _runs:
        _runs[key] = newton_run(qn, m, n, ls, memoize=memoize, chunk=chunk)
    return _runs[key]


@pytest.mark.parametrize("memoize", [1, 0])
@pytest.mark.parametrize("m,n,ls", LC.CASES)
def test_newton_cg_against_the_restatement(qn, m, n, ls, memoize):
    w = LC.window(m, n, ls)
    ref = LC.ref_case(m, n, ls)[0]
    run = _run(qn, m, n, ls, memoize, 8)
    assert len(run["trace"]) >= w and len(run["inner"]) == len(run["trace"])
    worst = 0.0
    for k in range(w):
        r, g = ref.trace[k], run["trace"][k]
        dx = float(np.linalg.norm(run["xs"][k] - ref.trace_x[k]) / max(1.0, np.linalg.norm(ref.trace_x[k])))
        worst = max(worst, dx)
        assert dx <= LC.GPU_TOL, (k, dx)
        assert g["n_evals"] == r["n_evals"] and g["ls_iters"] == r["ls_iters"], (k, g, r)
        assert (g["t"] == r["t"]) if ls == "bt" else (abs(g["t"] - r["t"]) <= LC.GPU_TOL * abs(r["t"])), (k, g["t"], r["t"])
        assert run["inner"][k] == ref.inner[k], (k, run["inner"], ref.inner)
    assert run["neg"][w - 1] == 0 and run["fb"][w - 1] == 0 and set(ref.why[:w]) <= {"tol", "cap"}
    if (m, n) in LC.CONVERGENCE:  # the convergence shapes reach 1e-7 in the restatement's iteration count, under both searches
        assert run["status"] == "ok" and LC.ref_case(m, n, ls)[2] == "ok" and run["k"] == ref.k, (run["k"], ref.k, run["status"])
    print(f"logistic NewtonCG {(m, n, ls)} memoize={memoize}: window {w} of {len(ref.trace)}, worst |x - x_ref| = {worst:.2e}, GPU k = {run['k']} ({run['status']})")


@pytest.mark.parametrize("m,n,ls", [(96, 64, "bt"), (257, 200, "wolfe"), (5, 2050, "bt")])
def test_the_chunk_never_changes_a_bit(qn, m, n, ls):
    base = _bits(_run(qn, m, n, ls, 1, 8))
    for chunk in (1, 3):
        assert _bits(_run(qn, m, n, ls, 1, chunk)) == base, chunk
    assert _bits(_run(qn, m, n, ls, 0, 8)) == base  # (memoize 0 evaluates the accepted point again: the same bits)


@pytest.mark.parametrize("m,n", LC.CONVERGENCE)
def test_convergence_and_one_weights_pass_per_iteration(qn, m, n):
    ref, _, ref_status = LC.ref_case(m, n, "bt")
    assert ref_status == "ok"
    run = _run(qn, m, n, "bt", 1, 8)
    assert run["status"] == "ok" and run["k"] == ref.k, (run["k"], ref.k)  # (every window is the whole run but its last iteration)
    pr = LC.problem(m, n)
    g = RL.truth_and_bound(pr[0], pr[1], pr[2], pr[3], run["x"])["g"]
    assert float(np.max(np.abs(g))) < LC.TOL
    assert run["hv"] == run["inner_total"] == sum(run["inner"])
    n_pad = 16 * ((n + 15) // 16)
    # obj_bytes = (evaluations + products + ONE weights pass per loop top) * 8 m n_pad, exactly: k outer iterations and the loop top that found the
    # run converged -- the weights' launches are the unpredicated ones of a batch -- where log-sum-exp counts two passes for each
    assert run["obj_bytes"] == (run["evals"] + run["hv"] + run["k"] + 1) * 8 * m * n_pad, (run["obj_bytes"], run["evals"], run["hv"], run["k"])
    assert run["path"] & qn._abi.PATH_NEWTON_CG and run["path"] & qn._abi.PATH_VECTOR


def test_negative_mu_takes_the_gradient(qn):
    ghg, gg = LC.neg_mu_curvature()
    assert ghg < 0.0 < gg  # chosen on the host: rule 4 at j = 0
    ref = LC.run_ref(3, 5, "bt", iters=3, mu=LC.NEG_MU)[0]
    assert ref.why[0] == "negcurv" and ref.inner[0] == 0
    run = newton_run(qn, 3, 5, "bt", iters=3, mu=LC.NEG_MU)
    assert run["neg"][0] >= 1 and run["inner"][0] == 0
    pr = LC.problem(3, 5)
    g0 = RL.logistic_fn(pr[0], pr[1], pr[2], LC.NEG_MU)(pr[4])[1]
    t0 = run["trace"][0]["t"]
    assert np.linalg.norm(run["xs"][0] - (pr[4] + t0 * -g0)) <= LC.GPU_TOL * max(1.0, np.linalg.norm(pr[4]))  # d = -g
    for k in range(min(3, len(ref.trace), len(run["trace"]))):
        assert run["inner"][k] == ref.inner[k] and run["trace"][k]["t"] == ref.trace[k]["t"] and run["trace"][k]["n_evals"] == ref.trace[k]["n_evals"], k


def test_two_calls_are_one(qn):
    one = newton_run(qn, 96, 64, "bt", iters=8)
    two = newton_run(qn, 96, 64, "bt", iters=4, calls=2)
    assert one["x"].tobytes() == two["x"].tobytes() and one["inner"] == two["inner"]
    assert [x.tobytes() for x in one["xs"]] == [x.tobytes() for x in two["xs"]]


# ---- 4. the rest of the family: the existing restatements on logistic_fn, and beside a host closure of it ----
def _family_gpu(qn, kind, m, n, oracle, iters):
    pr = LC.problem(m, n)
    lb, ub = LC.family_box(kind, n)
    if kind == "lbfgs":
        s, ls = qn.LBFGS(LC.FAMILY_TOL, pr[4], m=5, memoize=1), qn.StrongWolfe()
    elif kind == "cg":
        s, ls = qn.NonlinearCG(LC.FAMILY_TOL, pr[4], variant="pr+", memoize=1), qn.StrongWolfe(1e-4, 0.1)
    elif kind == "spg":
        s, ls = qn.SpectralProjectedGradient(LC.FAMILY_TOL, pr[4], oracle, lb, ub, memoize=1), qn.GLLQuadratic(1e-4, 10)
    else:
        s, ls = qn.ProjectedLBFGS(LC.FAMILY_TOL, pr[4], lb, ub, m=5, memoize=1), qn.BackTrackingB(1e-4, 0.5, lb, ub)
    s.set_trace(iters, with_x=True)
    try:
        s.minimize(ls, oracle, iters, 50)
    except qn.MaxIterReached:
        pass
    return s


@pytest.mark.parametrize("kind,m,n", LC.FAMILY_CASES)
def test_the_rest_of_the_family(qn, kind, m, n):
    ref, w = LC.family_licence(kind, m, n)
    assert w >= 4
    pr = LC.problem(m, n)
    fn = RL.logistic_fn(pr[0], pr[1], pr[2], pr[3])
    obj = _obj(qn, pr)
    dev = host = None
    try:
        dev = _family_gpu(qn, kind, m, n, obj, w)
        host = _family_gpu(qn, kind, m, n, lambda x: fn(x), w)
        ref_w = type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
        # t, n_evals, ls_iters, x at 1e-9 max(1, ||x||), gnorm at 1e-7: test_gpu_spg._compare, which test_gpu_lbfgs and test_gpu_cg use as well; then
        # what those two files add on top of it: `updated` equal and s_norm at 1e-9 max(1, s_norm) (test_gpu_lbfgs._compare_updates, test_gpu_cg._compare_cg)
        for run in (dev, host):
            _compare(run, ref_w, w)
            if kind != "spg":
                tr = run.trace()[0]
                assert [r["updated"] for r in tr[:w]] == ref.updated[:w]
                for k in range(w):
                    assert abs(tr[k]["s_norm"] - ref.trace[k]["s_norm"]) <= 1e-9 * max(1.0, ref.trace[k]["s_norm"]), k
        (dt, dx), (ht, hx) = dev.trace(), host.trace()
        for k in range(w):  # the device objective beside the host closure: equal decisions, x within the family's tolerance
            assert dt[k]["n_evals"] == ht[k]["n_evals"] and dt[k]["ls_iters"] == ht[k]["ls_iters"], k
            assert np.linalg.norm(dx[k] - hx[k]) <= 1e-9 * max(1.0, np.linalg.norm(hx[k])), k
        sd, sh = dev.stats(), host.stats()
        n_pad = 16 * ((n + 15) // 16)
        assert sd["obj_bytes"] == sd["oracle_evals"] * 8 * m * n_pad
        # TWO launches per evaluation: with memoize = 1 on both, the host closure's run makes the same launches but the objective's own (a device
        # objective's launches are unpredicated: the batch whose loop top ends the run may enqueue one evaluation that nothing asked for)
        extra = sd["launches"] - sh["launches"]
        print(f"logistic {kind} {(m, n)}: window {w}, launches device {sd['launches']} host {sh['launches']}, evaluations {sd['oracle_evals']}, closure calls {sh['oracle_calls']}")
        assert extra % 2 == 0 and extra // 2 - sd["oracle_evals"] in (0, 1), (extra, sd["oracle_evals"])
    finally:
        for run in (dev, host):
            if run is not None:
                run.close()
        obj.close()


# ---- 5. refusals: each ErrorInputParams with its message, before anything is launched ----
def test_creation_refusals(qn):
    rng = np.random.default_rng(5)
    a, y = rng.standard_normal((4, 3)), np.array([1.0, -1.0, 1.0, -1.0])
    for bad in (0.0, 2.0):
        yb = y.copy()
        yb[2] = bad
        with pytest.raises(qn.ErrorInputParams, match="2 y - 1"):
            qn.Logistic(a, yb, 0.5)
    for bad in (-1.0, float("nan"), float("inf")):
        w = np.ones(4)
        w[1] = bad
        with pytest.raises(qn.ErrorInputParams, match="negative or not finite"):
            qn.Logistic(a, y, 0.5, weights=w)
    with pytest.raises(qn.ErrorInputParams, match="not built for n_pad > 16384"):
        qn.Logistic(np.zeros((2, LC.TOO_WIDE)), np.array([1.0, -1.0]), 0.5)
    ok = qn.Logistic(a, y, -3.0)  # (any finite mu)
    ok.close()


def test_a_two_rank_context_is_refused(qn):
    def gather(send, recv):
        recv[:send.size] = send
        recv[send.size:] = send
    ctx = qn.Context(0, 0, 2, host_allgather=gather)  # (world = 2 through the host exchange, this rank alone)
    try:
        with pytest.raises(qn.ErrorInputParams, match="single-GPU"):
            qn.Logistic(np.ones((4, 3)), np.array([1.0, -1.0, 1.0, -1.0]), 0.5, ctx=ctx)
    finally:
        ctx.close()


def test_solver_and_entry_point_refusals(qn):
    pr = LC.problem(3, 5)
    obj = _obj(qn, pr)
    quad = qn.Quadratic(np.eye(5), np.zeros(5))
    x0 = pr[4]
    try:
        lb, ub = np.full(5, -1.0), np.full(5, 1.0)
        # the dense quasi-Newton family, the control-step solvers and Newton, then the projected Newton pair: refused before anything is launched
        refused = [(qn.BFGS(1e-8, x0), "Logistic"), (qn.DFP(1e-8, x0), "Logistic"), (qn.Broyden(1e-8, x0), "Logistic"),
                   (qn.GradientDescent(1e-8, x0), "Logistic"), (qn.CoordinateDescent(1e-8, x0), "Logistic"), (qn.Newton(1e-8, x0), "Logistic"),
                   (qn.ProjectedNewton(1e-8, x0, lb, ub), "Hessian not available")]
        for solver, message in refused:
            try:
                with pytest.raises(qn.ErrorInputParams, match=message):
                    solver.minimize(qn.BackTracking(1e-4, 0.5), obj, 5, 5)
                assert solver.stats()["launches"] == 0, type(solver).__name__
            finally:
                solver.close()
        # SpectralProjectedNewton's constructor calls the oracle once (spn.rs:40-46), through the same check: the refusal arrives there ...
        with pytest.raises(qn.ErrorInputParams, match="Hessian not available"):
            qn.SpectralProjectedNewton(1e-8, x0, obj, lb, ub)
        # ... and, built on a closure that carries its Hessian, it refuses the Logistic without a launch more than it had made
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
        with pytest.raises(qn.ErrorInputParams, match="dense Hessian of a logistic objective"):
            obj.hessian(x0)
        with pytest.raises(qn.ErrorInputParams, match="hess_vec_at"):
            obj.hess_vec(x0)
        tn = qn.NewtonCG(1e-7, x0)
        with pytest.raises(qn.ErrorInputParams, match="LogSumExp or Logistic"):
            tn.minimize(qn.BackTracking(1e-4, 0.5), quad, 5, 5)
        with pytest.raises(qn.ErrorInputParams, match="BackTracking or StrongWolfe"):
            tn.minimize(qn.GLLQuadratic(1e-4, 10), obj, 5, 5)
        tn.close()
    finally:
        obj.close()
        quad.close()
