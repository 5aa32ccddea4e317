"""GPU tests of the device sparse multinomial objective (qn.SparseMultinomial; kernels csrc/qn_sparse_multinomial.hip.h): the evaluation, the
probabilities and the Hessian-vector product against np.longdouble on the densified matrix inside the derived bounds of tests/ref_multinomial.py (C = 8
is a cap, not a measurement) at every shape, scale and weighting of tests/sparse_multinomial_cases.py and with every lane count forced on both passes;
bit-for-bit repeatability; int32 and int64 index arrays; the dense Multinomial beside it; NewtonCG against the restatement inside the windows
tests/test_ref_sparse_multinomial.py licenses; the rest of the O(n) family against the existing restatements and beside a host closure of the same
function; and the refusals.

MEASURED on one MI355X, one run (the largest |error| / bound over all shapes, scales, weightings and lane counts, printed by the tests):
f 0.115, g 0.331, P 0.854, H v 0.331, v'Hv 0.093.  P's largest is a subnormal p_k = 8e-322 at (4096, 300, 4), scale 30, whose bound is the float64
step 2^-1074 (the float64 restatement on the CPU has the same ratio there); at every other point P stays below 0.25."""
import numpy as np
import pytest

import ref_multinomial as RM
import sparse_multinomial_cases as SM
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
LD = np.longdouble
_worst = {}


def _obj(qn, pr, mu=None, ctx=None, dtype=None):
    ip, ix = (pr["indptr"], pr["indices"]) if dtype is None else (pr["indptr"].astype(dtype), pr["indices"].astype(dtype))
    return qn.SparseMultinomial(ip, ix, pr["data"], pr["y"], pr["k"], pr["mu"] if mu is None else mu, pr["a"].shape[1], weights=pr["w"], ctx=ctx)


def _check_point(obj, pr, x, truth, label, product=True):
    ev = obj(x)
    got = dict(f=ev.f(), g=ev.g(), p=obj.probabilities(x))
    if product:
        got["q"], got["c"] = obj.hess_vec_at(x, pr["v"])
    r = RM.ratios(got, truth)
    for key, val in r.items():
        _worst[key] = max(_worst.get(key, 0.0), val)
    print(f"sparse multinomial {label}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, (label, r)
    if product:  # v'Hv matches the returned vector: the shares' sum of v_j q_j, N products in another order
        v, q = pr["v"], got["q"]
        assert abs(LD(got["c"]) - np.sum(v.astype(LD) * q.astype(LD))) <= LD(RM.gamma(v.size + 2)) * np.sum(np.abs(v * q).astype(LD))
    return got


# ---- 1. the evaluation, the probabilities and the product ----
@pytest.mark.parametrize("m,n,k", SM.SHAPES)
def test_evaluation_and_product_inside_the_bounds(qn, m, n, k):
    """f, g, P, H v and v'Hv against longdouble at the scales 1e-3, 1 and 30 on the weighted problem (masked rows wherever the draw put them), and at
    scale 1 with unit weights and with the first and the last row of a workgroup's cut masked"""
    for kind, scales in [("weighted", SM.SCALES), ("unit", [1.0]), ("edges", [1.0])]:
        obj = _obj(qn, SM.problem(m, n, k, kind))
        try:
            for scale in scales:
                pr, x, truth = SM.truth_at(m, n, k, scale, kind)
                _check_point(obj, pr, x, truth, f"{(m, n, k)} {kind} scale {scale:g}")
        finally:
            obj.close()
    print("sparse multinomial worst so far:", {key: f"{v:.3f}" for key, v in _worst.items()})


@pytest.mark.parametrize("m,n,k", [(40, 65, 5), (96, 64, 16)])
def test_every_lane_count_on_both_passes(qn, m, n, k):
    """every L forced on the row pass and on the column pass (the class lanes shrink to 64 / L: more class slots, then class blocks); the bits may
    differ, the bounds hold; 0 restores the automatic choice and its bits"""
    pr, x, truth = SM.truth_at(m, n, k, 1.0)
    obj = _obj(qn, pr)
    try:
        auto = obj.lanes
        base = _check_point(obj, pr, x, truth, f"{(m, n, k)} automatic lanes {auto}")
        for lr, lc in [(L, L) for L in SM.LANES] + [(1, 64), (64, 1)]:
            obj.set_lanes(lr, lc)
            assert obj.lanes == (lr, lc)
            got = _check_point(obj, pr, x, truth, f"{(m, n, k)} lanes {(lr, lc)}")
            if (m, n) == (40, 65):  # the empty column: g_kj = mu x_kj exactly, for every class
                assert np.array_equal(got["g"].reshape(k, n)[:, 64], pr["mu"] * x.reshape(k, n)[:, 64])
        obj.set_lanes(0, 0)
        assert obj.lanes == auto
        again = obj(x)
        assert again.f() == base["f"] and again.g().tobytes() == base["g"].tobytes()
        for bad in ((3, 1), (1, 128), (-1, 1)):
            with pytest.raises(qn.ErrorInputParams, match="lanes must be"):
                obj.set_lanes(*bad)
    finally:
        obj.close()


def test_an_empty_row_and_an_absent_class(qn):
    """(40, 65, 5): row 0 has no entry -- its margins are 0, its loss w log K, p = 1 / K; no row carries class 4"""
    pr, x, _ = SM.truth_at(40, 65, 5, 1.0)
    assert pr["indptr"][1] == 0 and not np.any(pr["y"] == 4)
    one = dict(pr, w=np.where(np.arange(40) == 0, 3.0, 0.0))
    obj = _obj(qn, one)
    try:
        ev, p = obj(x), obj.probabilities(x)
        assert abs(ev.f() - (3.0 * np.log(5.0) + 0.25 * float(x @ x))) <= 1e-13 * ev.f() and np.array_equal(ev.g(), pr["mu"] * x)
        assert np.array_equal(p[0], np.full(5, 0.2)) and not p[1:].any()
    finally:
        obj.close()


def test_saturated_margins(qn):
    """a margin spread of 1600: f is finite and inside its bound, the losers' probabilities are exactly 0, the masked row adds nothing"""
    pr, x, spread = SM.saturated_problem()
    truth = RM.truth_and_bound(pr["a"], pr["y"], pr["w"], pr["k"], pr["mu"], x)
    obj = _obj(qn, pr)
    try:
        ev, p = obj(x), obj.probabilities(x)
        r = RM.ratios(dict(f=ev.f(), g=ev.g(), p=p), truth)
        assert np.isfinite(ev.f()) and ev.f() > spread and max(r.values()) <= 1.0, (ev.f(), r)
        assert p[0, 1] == 0.0 and p[0, 2] == 0.0 and p[0, 0] == 1.0 and not p[2].any()
    finally:
        obj.close()


# ---- 3. the same bits ----
@pytest.mark.parametrize("m,n,k", [(96, 64, 16), (2050, 7, 3), (5, 2050, 4), (7, 9, 300), (4096, 300, 4), (64, 20000, 5)])
def test_same_bits_from_call_to_call_and_object_to_object_and_index_width(qn, m, n, k):
    pr, x, _ = SM.truth_at(m, n, k, 1.0)
    one, two = _obj(qn, pr), _obj(qn, pr, dtype=np.int64)
    try:
        a1, a2, b1 = one(x), one(x), two(x)
        assert a1.f() == a2.f() == b1.f() and a1.g().tobytes() == a2.g().tobytes() == b1.g().tobytes()
        (q1, c1), (q2, c2), (q3, c3) = one.hess_vec_at(x, pr["v"]), one.hess_vec_at(x, pr["v"]), two.hess_vec_at(x, pr["v"])
        assert c1 == c2 == c3 and q1.tobytes() == q2.tobytes() == q3.tobytes()
        assert one.probabilities(x).tobytes() == two.probabilities(x).tobytes()
        none, c4 = one.hess_vec_at(x, pr["v"], download=False)
        assert none is None and c4 == c1
        one(30.0 * x)  # an evaluation elsewhere writes the trial buffer: the product at x is still the product at x
        q5, c5 = one.hess_vec_at(x, pr["v"])
        assert q5.tobytes() == q1.tobytes() and c5 == c1
    finally:
        one.close()
        two.close()


def test_from_scipy_and_other_index_types(qn):
    import scipy.sparse as sp
    pr, x, _ = SM.truth_at(96, 64, 16, 1.0)
    base = _obj(qn, pr)
    coo = sp.coo_matrix(sp.csr_matrix((pr["data"], pr["indices"], pr["indptr"]), shape=(96, 64)))
    objs = [qn.SparseMultinomial.from_scipy(coo, pr["y"], 16, pr["mu"], weights=pr["w"]),
            qn.SparseMultinomial(pr["indptr"].astype(np.int64), pr["indices"], pr["data"], pr["y"], 16, pr["mu"], 64, weights=pr["w"]),  # a mixed pair
            qn.SparseMultinomial(pr["indptr"].astype(np.uint16), pr["indices"].astype(np.uint16), pr["data"], pr["y"].astype(np.float64), 16, pr["mu"], 64, weights=pr["w"])]
    try:
        ref = base(x)
        for o in objs:
            ev = o(x)
            assert ev.f() == ref.f() and ev.g().tobytes() == ref.g().tobytes()
            assert (o.n_classes, o.m, o.n, o.n_features) == (16, 96, 16 * 64, 64)
    finally:
        for o in objs + [base]:
            o.close()


# ---- 4. the dense Multinomial beside it ----
def test_the_dense_multinomial_beside_it(qn):
    """the dense Multinomial on the densified (96, 64, 16) problem: both inside the bounds of the same truth (bit equality is not required)"""
    pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
    sparse, dense = _obj(qn, pr), qn.Multinomial(pr["a"], pr["y"], 16, pr["mu"], weights=pr["w"])
    try:
        for name, obj in (("sparse", sparse), ("dense", dense)):
            ev = obj(x)
            q, c = obj.hess_vec_at(x, pr["v"])
            r = RM.ratios(dict(f=ev.f(), g=ev.g(), p=obj.probabilities(x), q=q, c=c), truth)
            print(f"{name} (96, 64, 16): " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
            assert max(r.values()) <= 1.0, (name, r)
    finally:
        sparse.close()
        dense.close()


# ---- 5. the structure ----
def test_the_structure_the_shapes_are_for(qn):
    for (m, n, k), long_rows, long_cols in [((5, 2050, 4), 1, 0), ((2050, 7, 3), 0, 1), ((96, 64, 16), 0, 0), ((64, 20000, 5), 0, 0), ((17, 8, 17), 0, 0),
                                            ((9, 7, 65), 0, 0), ((5, 4, 600), 0, 0), ((20, 1025, 16), 0, 0)]:
        pr = SM.problem(m, n, k)
        obj = _obj(qn, pr)
        try:
            nnz = pr["data"].size
            assert (obj.m, obj.n, obj.n_classes, obj.nnz, obj.n_long_rows, obj.n_long_cols) == (m, n * k, k, nnz, long_rows, long_cols)
            assert obj.kp == SM.kp(k) and obj.kp >= k
            assert obj.lanes == (SM.auto_lanes(m, nnz, k), SM.auto_lanes(n, nnz, k))
        finally:
            obj.close()
    assert [SM.kp(k) for k in (2, 3, 4, 5, 16, 17, 64, 65, 300, 600)] == [2, 4, 4, 8, 16, 32, 64, 80, 304, 608]


# ---- 6. NewtonCG against the restatement, inside the licensed windows ----
def _ls(qn, kind):
    return qn.StrongWolfe(*SM.WOLFE) if kind == "wolfe" else qn.BackTracking(1e-4, 0.5)


def _bytes_model(pr):
    (m, n), k = pr["a"].shape, pr["k"]
    kp = SM.kp(k)
    base = 24 * pr["data"].size + 4 * (m + 1) + 4 * (n + 1) + 24 * m * kp + 32 * n * kp + 24 * n * k
    return base + 12 * m, base + 8 * m  # (one evaluation, one product)


def newton_run(qn, m, n, k, ls, iters=SM.ITERS, memoize=1, chunk=8, mu=None, calls=1):
    pr = SM.problem(m, n, k)
    obj = _obj(qn, pr, mu)
    s = qn.NewtonCG(SM.TOL, pr["x0"], chunk=chunk, memoize=memoize)
    out = dict(trace=[], xs=[], inner=[], neg=[], fb=[], hv=0, inner_total=0, status="ok", k=0)
    try:
        for _ in range(calls):
            s.set_trace(iters, with_x=True)
            rec = []
            try:
                s.minimize(_ls(qn, ls), obj, iters, SM.MAX_LS, callback=lambda sv: rec.append((sv.inner_iterations()[0], sv.negative_curvature(), sv.fallbacks())))
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


def _run(qn, m, n, k, ls, memoize, chunk):
    key = (m, n, k, ls, memoize, chunk)
    if key not in _runs:
        _runs[key] = newton_run(qn, m, n, k, ls, memoize=memoize, chunk=chunk)
    return _runs[key]


@pytest.mark.parametrize("memoize", [1, 0])
@pytest.mark.parametrize("m,n,k,ls", SM.CASES)
def test_newton_cg_against_the_restatement(qn, m, n, k, ls, memoize):
    """every decision of the restatement inside the licensed window, and 1e-7 in the restatement's outer iteration count"""
    w = SM.window(m, n, k, ls)
    ref, _, ref_status = SM.ref_case(m, n, k, ls)
    run = _run(qn, m, n, k, ls, memoize, 8)
    assert len(run["trace"]) >= w and len(run["inner"]) == len(run["trace"])
    worst = 0.0
    for i in range(w):
        r, g = ref.trace[i], run["trace"][i]
        dx = float(np.linalg.norm(run["xs"][i] - ref.trace_x[i]) / max(1.0, np.linalg.norm(ref.trace_x[i])))
        worst = max(worst, dx)
        assert dx <= SM.GPU_TOL, (i, dx)
        assert g["n_evals"] == r["n_evals"] and g["ls_iters"] == r["ls_iters"], (i, g, r)
        assert (g["t"] == r["t"]) if ls == "bt" else (abs(g["t"] - r["t"]) <= SM.GPU_TOL * abs(r["t"])), (i, g["t"], r["t"])
        assert run["inner"][i] == ref.inner[i], (i, run["inner"], ref.inner)
    assert run["neg"][w - 1] == 0 and run["fb"][w - 1] == 0 and set(ref.why[:w]) <= {"tol", "cap"}
    assert run["status"] == "ok" and ref_status == "ok" and run["k"] == ref.k, (run["k"], ref.k, run["status"])
    print(f"sparse multinomial NewtonCG {(m, n, k, ls)} memoize={memoize}: window {w} of {len(ref.trace)}, worst |x - x_ref| = {worst:.2e}, GPU k = {run['k']} "
          f"({run['status']}), inner {sum(run['inner'])}")


@pytest.mark.parametrize("m,n,k,ls", [(96, 16, 4, "bt"), (257, 40, 5, "wolfe"), (20, 1025, 16, "bt")])
def test_the_chunk_never_changes_a_bit(qn, m, n, k, ls):
    base = _bits(_run(qn, m, n, k, ls, 1, 8))
    for chunk in (1, 3):
        assert _bits(_run(qn, m, n, k, ls, 1, chunk)) == base, chunk
    assert _bits(_run(qn, m, n, k, ls, 0, 8)) == base  # (memoize 0 evaluates the accepted point again: the same bits)


@pytest.mark.parametrize("m,n,k", SM.NEWTON_SHAPES)
def test_convergence_and_one_weights_pass_per_iteration(qn, m, n, k):
    ref, _, ref_status = SM.ref_case(m, n, k, "bt")
    assert ref_status == "ok"
    run = _run(qn, m, n, k, "bt", 1, 8)
    assert run["status"] == "ok" and run["k"] == ref.k, (run["k"], ref.k)
    pr = SM.problem(m, n, k)
    g = RM.truth_and_bound(pr["a"], pr["y"], pr["w"], k, pr["mu"], run["x"])["g"]
    assert float(np.max(np.abs(g))) < SM.TOL
    assert run["hv"] == run["inner_total"] == sum(run["inner"])
    # obj_bytes = (evaluations + ONE weights pass per loop top) * an evaluation's bytes + products * a product's bytes, exactly
    eval_bytes, product_bytes = _bytes_model(pr)
    assert run["obj_bytes"] == (run["evals"] + run["k"] + 1) * eval_bytes + run["hv"] * product_bytes, (run["obj_bytes"], run["evals"], run["hv"], run["k"])
    assert run["path"] & qn._abi.PATH_NEWTON_CG and run["path"] & qn._abi.PATH_VECTOR
    print(f"sparse multinomial NewtonCG {(m, n, k)} bt: outer {run['k']}, inner {run['inner_total']}, evaluations {run['evals']}, weights passes {run['k'] + 1}, launches {run['launches']}")


def test_negative_mu_takes_the_gradient(qn):
    ghg, gg = SM.neg_mu_curvature()
    assert ghg < 0.0 < gg  # chosen on the host: rule 4 at j = 0
    ref = SM.run_ref(*SM.NEG_SHAPE, "bt", iters=3, mu=SM.NEG_MU)[0]
    assert ref.why[0] == "negcurv" and ref.inner[0] == 0
    run = newton_run(qn, *SM.NEG_SHAPE, "bt", iters=3, mu=SM.NEG_MU)
    assert run["neg"][0] >= 1 and run["inner"][0] == 0
    pr = SM.problem(*SM.NEG_SHAPE)
    g0 = SM.csr_functions(pr, SM.NEG_MU)[0](pr["x0"])[1]
    t0 = run["trace"][0]["t"]
    assert np.linalg.norm(run["xs"][0] - (pr["x0"] + t0 * -g0)) <= SM.GPU_TOL * max(1.0, np.linalg.norm(pr["x0"]))  # d = -g
    for i in range(min(3, len(ref.trace), len(run["trace"]))):
        assert run["inner"][i] == ref.inner[i] and run["trace"][i]["t"] == ref.trace[i]["t"] and run["trace"][i]["n_evals"] == ref.trace[i]["n_evals"], i


def test_two_calls_are_one(qn):
    one = newton_run(qn, 96, 16, 4, "bt", iters=8)
    two = newton_run(qn, 96, 16, 4, "bt", iters=4, calls=2)
    assert one["x"].tobytes() == two["x"].tobytes() and one["inner"] == two["inner"]
    assert [x.tobytes() for x in one["xs"]] == [x.tobytes() for x in two["xs"]]


# ---- 7. the rest of the family: the existing restatements on the same function, and beside a host closure of it ----
def _family_gpu(qn, kind, m, n, k, oracle, iters):
    pr = SM.problem(m, n, k)
    x0 = pr["x0"]
    lb, ub = SM.family_box(kind, n * k)
    if kind == "lbfgs":
        s, ls = qn.LBFGS(SM.FAMILY_TOL, x0, m=5, memoize=1), qn.StrongWolfe()
    elif kind == "cg":
        s, ls = qn.NonlinearCG(SM.FAMILY_TOL, x0, variant="pr+", memoize=1), qn.StrongWolfe(1e-4, 0.1)
    elif kind == "spg":
        s, ls = qn.SpectralProjectedGradient(SM.FAMILY_TOL, x0, oracle, lb, ub, memoize=1), qn.GLLQuadratic(1e-4, 10)
    else:
        s, ls = qn.ProjectedLBFGS(SM.FAMILY_TOL, x0, lb, ub, m=5, memoize=1), qn.BackTrackingB(1e-4, 0.5, lb, ub)
    s.set_trace(iters, with_x=True)
    try:
        s.minimize(ls, oracle, iters, 50)
    except qn.MaxIterReached:
        pass
    return s


@pytest.mark.parametrize("kind,m,n,k", SM.FAMILY_CASES)
def test_the_rest_of_the_family(qn, kind, m, n, k):
    ref, w = SM.family_licence(kind, m, n, k)
    assert w >= 4
    pr = SM.problem(m, n, k)
    fn = RM.multinomial_fn(pr["a"], pr["y"], pr["w"], k, pr["mu"])
    obj = _obj(qn, pr)
    dev = host = None
    try:
        dev = _family_gpu(qn, kind, m, n, k, obj, w)
        host = _family_gpu(qn, kind, m, n, k, lambda x: fn(x), w)
        ref_w = type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
        for run in (dev, host):  # test_gpu_multinomial's comparison: test_gpu_spg._compare, then `updated` and s_norm for the methods that have them
            _compare(run, ref_w, w)
            if kind != "spg":
                tr = run.trace()[0]
                assert [r["updated"] for r in tr[:w]] == ref.updated[:w]
                for i in range(w):
                    assert abs(tr[i]["s_norm"] - ref.trace[i]["s_norm"]) <= 1e-9 * max(1.0, ref.trace[i]["s_norm"]), i
        (dt, dx), (ht, hx) = dev.trace(), host.trace()
        for i in range(w):  # the device objective beside the host closure: equal decisions, x within the family's tolerance
            assert dt[i]["n_evals"] == ht[i]["n_evals"] and dt[i]["ls_iters"] == ht[i]["ls_iters"], i
            assert np.linalg.norm(dx[i] - hx[i]) <= 1e-9 * max(1.0, np.linalg.norm(hx[i])), i
        sd, sh = dev.stats(), host.stats()
        assert sd["obj_bytes"] == sd["oracle_evals"] * _bytes_model(pr)[0]
        # FIVE launches per evaluation (a device objective's launches are unpredicated: the batch whose loop top ends the run may enqueue one
        # evaluation that nothing asked for)
        extra = sd["launches"] - sh["launches"]
        print(f"sparse multinomial {kind} {(m, n, k)}: window {w}, launches device {sd['launches']} host {sh['launches']}, evaluations {sd['oracle_evals']}, closure calls {sh['oracle_calls']}")
        assert extra % 5 == 0 and extra // 5 - sd["oracle_evals"] in (0, 1), (extra, sd["oracle_evals"])
    finally:
        for run in (dev, host):
            if run is not None:
                run.close()
        obj.close()


# ---- 8. refusals: each ErrorInputParams with its message, before anything is launched ----
def test_creation_refusals(qn):
    pr = SM.problem(3, 5, 3)
    ip, ix, da, y = pr["indptr"], pr["indices"], pr["data"], pr["y"]
    assert da.size >= 4 and np.diff(ip).max() >= 2
    for bad in (3, -1, 1.5):
        yb = y.astype(np.float64)
        yb[2] = bad
        with pytest.raises(qn.ErrorInputParams, match=r"labels\[2\]"):
            qn.SparseMultinomial(ip, ix, da, yb, 3, 0.5, 5)
    for bad in (-1.0, float("nan"), float("inf")):
        w = np.ones(3)
        w[1] = bad
        with pytest.raises(qn.ErrorInputParams, match=r"weights\[1\] is negative or not finite"):
            qn.SparseMultinomial(ip, ix, da, y, 3, 0.5, 5, weights=w)
    with pytest.raises(qn.ErrorInputParams, match="mu must be finite"):
        qn.SparseMultinomial(ip, ix, da, y, 3, float("inf"), 5)
    with pytest.raises(qn.ErrorInputParams, match="fewer than 2 classes"):
        qn.SparseMultinomial(ip, ix, da, np.zeros(3), 1, 0.5, 5)
    i = int(np.argmax(np.diff(ip) >= 2))  # a row with two entries
    swapped = ix.copy()
    swapped[ip[i]], swapped[ip[i] + 1] = ix[ip[i] + 1], ix[ip[i]]
    with pytest.raises(qn.ErrorInputParams, match="strictly increasing"):
        qn.SparseMultinomial(ip, swapped, da, y, 3, 0.5, 5)
    dup = ix.copy()
    dup[ip[i] + 1] = ix[ip[i]]
    with pytest.raises(qn.ErrorInputParams, match="strictly increasing"):
        qn.SparseMultinomial(ip, dup, da, y, 3, 0.5, 5)
    with pytest.raises(qn.ErrorInputParams, match=r"outside \[0, n\)"):  # a column >= n
        qn.SparseMultinomial(ip, ix, da, y, 3, 0.5, int(ix.max()))
    with pytest.raises(qn.ErrorInputParams, match="do not match"):
        qn.SparseMultinomial(ip[:-1], ix, da, y, 3, 0.5, 5)
    with pytest.raises(qn.ErrorInputParams, match="empty shape"):
        qn.SparseMultinomial(ip, ix, da, y, 3, 0.5, 0)
    with pytest.raises(qn.ErrorInputParams, match="K n must not exceed"):
        qn.SparseMultinomial(ip, ix, da, y, 1 << 29, 0.5, 5)
    ok = qn.SparseMultinomial(ip, ix, da, y, 3, -3.0, 5)  # (any finite mu)
    ok.close()
    empty = qn.SparseMultinomial(np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), y, 3, 0.5, 5)  # nnz = 0: f = sum w log K + mu/2 ||x||^2
    try:
        ev = empty(pr["x0"])
        assert abs(ev.f() - (3.0 * np.log(3.0) + 0.25 * float(pr["x0"] @ pr["x0"]))) <= 1e-14 * ev.f() and np.array_equal(ev.g(), 0.5 * pr["x0"])
    finally:
        empty.close()


def test_a_two_rank_context_is_refused(qn):
    def gather(send, recv):
        recv[:send.size] = send
        recv[send.size:] = send
    ctx = qn.Context(0, 0, 2, host_allgather=gather)  # (world = 2 through the host exchange, this rank alone)
    try:
        with pytest.raises(qn.ErrorInputParams, match="single-GPU"):
            _obj(qn, SM.problem(3, 5, 3), ctx=ctx)
    finally:
        ctx.close()


def test_solver_and_entry_point_refusals(qn):
    pr = SM.problem(3, 5, 3)
    obj = _obj(qn, pr)
    quad = qn.Quadratic(np.eye(15), np.zeros(15))
    x0 = pr["x0"]
    try:
        lb, ub = np.full(15, -1.0), np.full(15, 1.0)
        # the dense quasi-Newton family, the control-step solvers and Newton, then the projected Newton pair: refused before anything is launched
        refused = [(qn.BFGS(1e-8, x0), "SparseMultinomial"), (qn.DFP(1e-8, x0), "SparseMultinomial"), (qn.Broyden(1e-8, x0), "SparseMultinomial"),
                   (qn.GradientDescent(1e-8, x0), "SparseMultinomial"), (qn.CoordinateDescent(1e-8, x0), "SparseMultinomial"),
                   (qn.Newton(1e-8, x0), "SparseMultinomial"),
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
        spn = qn.SpectralProjectedNewton(1e-8, x0, lambda p: (0.5 * float(p @ p), p, np.eye(15)), lb, ub)
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
        with pytest.raises(qn.ErrorInputParams, match="no dense rows / Hessian"):
            obj.hessian(x0)
        with pytest.raises(qn.ErrorInputParams, match="sparse multinomial objective depends on x"):
            obj.hess_vec(x0)
        with pytest.raises(qn.ErrorInputParams, match="no dense rows / Hessian"):
            obj.rows(0, 1)
        with pytest.raises(qn.ErrorInputParams, match="qn_sparse_multinomial_info"):
            qn.SparseQuadratic._info(obj)  # (qn_objective_sparse_info on this handle)
        with pytest.raises(qn.ErrorInputParams, match="not a multinomial objective"):
            qn.Multinomial.set_kernel(obj, 1)
        with pytest.raises(qn.ErrorInputParams, match="not a multinomial objective"):
            qn.Multinomial.probabilities(obj, x0)
        with pytest.raises(qn.ErrorInputParams, match="not a sparse logistic"):
            qn.SparseLogistic._info(obj)
        with pytest.raises(qn.ErrorInputParams, match="belong to a sparse logistic"):
            qn.SparseLogistic.set_lanes(obj, 1, 1)
        with pytest.raises(qn.ErrorInputParams, match="not a sparse multinomial"):
            qn.SparseMultinomial._info(quad)
        with pytest.raises(qn.ErrorInputParams, match="belong to a sparse multinomial"):
            qn.SparseMultinomial.set_lanes(quad, 1, 1)
        tn = qn.NewtonCG(1e-7, x0)
        with pytest.raises(qn.ErrorInputParams, match="BackTracking or StrongWolfe"):
            tn.minimize(qn.GLLQuadratic(1e-4, 10), obj, 5, 5)
        assert tn.stats()["launches"] == 0
        tn.close()
        boxed = qn.NewtonCG(1e-7, x0)  # (a box under NewtonCG: out of scope, whatever the objective)
        with pytest.raises(qn.ErrorInputParams, match="unbounded only"):
            boxed.minimize(qn.StrongWolfe().with_lower_bound(lb), obj, 5, 5)
        boxed.close()
    finally:
        obj.close()
        quad.close()
