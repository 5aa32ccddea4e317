"""GPU tests of the device sparse logistic objective (qn.SparseLogistic; kernels csrc/qn_sparse_logistic.hip.h): the evaluation and the Hessian-vector
product against np.longdouble on the densified matrix inside the derived bounds of tests/ref_logistic.py (C = 8 is a cap, not a measurement) at every
shape, scale and mask of tests/sparse_logistic_cases.py and with every lane count forced on both passes; bit-for-bit repeatability; int32 and int64
index arrays; the dense Logistic beside it; NewtonCG against the restatement inside the windows tests/test_ref_sparse_logistic.py licenses; the rest of
the O(n) family against the existing restatements and beside a host closure of the same function; and the refusals.

MEASURED on one MI355X (the largest |error| / bound over all shapes, scales, weightings and lane counts, printed by the tests): f 0.076,
g 0.185, H v 0.152, v'Hv 0.141.

d has no entry point of its own: it is held to its bound through H v, whose bound propagates d's (ref_logistic.truth_and_bound), and directly on the
CPU restatement (tests/test_ref_sparse_logistic.py)."""
import numpy as np
import pytest

import logistic_cases as LC
import ref_logistic as RL
import sparse_logistic_cases as SC
from test_gpu_spg import _compare

pytestmark = pytest.mark.gpu
LD = np.longdouble
_worst = {}


def _obj(qn, pr, mu=None, ctx=None, dtype=None):
    ip, ix = (pr["indptr"], pr["indices"]) if dtype is None else (pr["indptr"].astype(dtype), pr["indices"].astype(dtype))
    return qn.SparseLogistic(ip, ix, pr["data"], pr["y"], pr["mu"] if mu is None else mu, pr["a"].shape[1], weights=pr["w"], ctx=ctx)


def _note(key, ratios):
    for k, r in ratios.items():
        _worst[(key, k)] = max(_worst.get((key, k), 0.0), r)


def _check_point(obj, pr, x, truth, label, product=True):
    ev = obj(x)
    got = dict(f=ev.f(), g=ev.g())
    if product:
        got["q"], got["c"] = obj.hess_vec_at(x, pr["v"])
    r = RL.ratios(got, truth)
    _note("all", r)
    print(f"sparse logistic {label}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, (label, r)
    if product:  # v'Hv matches the returned vector: the shares' sum of v_j q_j, n products in another order
        v, q = pr["v"], got["q"]
        assert abs(LD(got["c"]) - np.sum(v.astype(LD) * q.astype(LD))) <= LD(RL.gamma(v.size + 2)) * np.sum(np.abs(v * q).astype(LD))
    return got


# ---- 1. the evaluation and the product ----
@pytest.mark.parametrize("m,n", SC.SHAPES)
def test_evaluation_and_product_inside_the_bounds(qn, m, n):
    """f, g, H v and v'Hv against longdouble at the scales 1e-3, 1 and 30 on the weighted problem (masked rows wherever the draw put them), and at scale
    1 with unit weights and with the first and the last row of a workgroup's cut masked"""
    kinds = [("weighted", SC.SCALES), ("unit", [1.0]), ("edges", [1.0])] + ([("full", [1.0])] if (m, n) == (40, 65) else [])
    for kind, scales in kinds:
        obj = _obj(qn, SC.problem(m, n, kind))
        try:
            for scale in scales:
                pr, x, truth = SC.truth_at(m, n, scale, kind)
                _check_point(obj, pr, x, truth, f"{(m, n)} {kind} scale {scale:g}")
        finally:
            obj.close()
    print("sparse logistic worst so far:", {k[1]: f"{v:.3f}" for k, v in _worst.items()})


def test_the_structure_the_shapes_are_for(qn):
    for (m, n), long_rows, long_cols in [((5, 2050), 1, 0), ((2050, 7), 0, 1), ((96, 64), 0, 0), ((64, 20000), 0, 0)]:
        pr = SC.problem(m, n)
        obj = _obj(qn, pr)
        try:
            assert (obj.m, obj.n, obj.nnz, obj.n_long_rows, obj.n_long_cols) == (m, n, pr["data"].size, long_rows, long_cols)
            lr, lc = obj.lanes
            for lanes, rows in ((lr, m), (lc, n)):  # the automatic choice: the largest power of two at most half the mean row length
                assert lanes in SC.LANES and (lanes == 1 or 2 * lanes <= pr["data"].size / rows) and (lanes == 64 or 4 * lanes > pr["data"].size / rows)
        finally:
            obj.close()


def test_every_lane_count_on_both_passes(qn):
    """(40, 65), with an empty row and an empty column: every L forced on the row pass and on the column pass; the bits may differ, the bounds hold;
    0 restores the automatic choice and its bits"""
    pr, x, truth = SC.truth_at(40, 65, 1.0)
    obj = _obj(qn, pr)
    try:
        auto = obj.lanes
        base = _check_point(obj, pr, x, truth, "(40, 65) automatic lanes")
        assert base["g"][64] == pr["mu"] * x[64]  # the empty column: g_j = mu x_j exactly
        for lr, lc in [(L, L) for L in SC.LANES] + [(1, 64), (64, 1)]:
            obj.set_lanes(lr, lc)
            assert obj.lanes == (lr, lc)
            got = _check_point(obj, pr, x, truth, f"(40, 65) lanes {(lr, lc)}")
            assert got["g"][64] == pr["mu"] * x[64]
        obj.set_lanes(0, 0)
        assert obj.lanes == auto
        again = obj(x)
        assert again.f() == base["f"] and again.g().tobytes() == base["g"].tobytes()
        for bad in ((3, 1), (1, 128), (-1, 1)):
            with pytest.raises(qn.ErrorInputParams, match="lanes must be"):
                obj.set_lanes(*bad)
    finally:
        obj.close()
    # the empty row: its margin is 0, its loss w log 2, alone in a problem of one live row
    one = dict(pr, w=np.where(np.arange(40) == 0, 3.0, 0.0))
    obj = _obj(qn, one)
    try:
        ev = obj(x)
        assert abs(ev.f() - (3.0 * np.log(2.0) + 0.25 * float(x @ x))) <= 1e-13 * ev.f() and np.array_equal(ev.g(), pr["mu"] * x)
    finally:
        obj.close()


def test_saturated_margins(qn):
    """margins of -800, +800, +800 (masked) and 0.5: f is finite and inside its bound, s and d are exactly 0 on the saturated side"""
    pr, x, _ = SC.saturated_problem()
    truth = RL.truth_and_bound(pr["a"], pr["y"], pr["w"], pr["mu"], x)
    obj = _obj(qn, pr)
    try:
        ev = obj(x)
        r = RL.ratios(dict(f=ev.f(), g=ev.g()), truth)
        assert np.isfinite(ev.f()) and ev.f() > 800.0 and r["f"] <= 1.0 and r["g"] <= 1.0, (ev.f(), r)
        assert ev.g()[1] == pr["mu"] * x[1]
        for j in range(3):
            e = np.zeros(3)
            e[j] = 1.0
            q, c = obj.hess_vec_at(x, e)
            d_j = float(truth["d"][3]) * 0.25 if j == 2 else 0.0  # (row 3 alone has curvature: d_3 a_3j^2)
            assert np.array_equal(q[:2], pr["mu"] * e[:2]) and abs(q[2] - (d_j + pr["mu"] * e[2])) <= 1e-15 and c == q[j], (j, q, c)
    finally:
        obj.close()


@pytest.mark.parametrize("m,n", [(96, 64), (2050, 7), (5, 2050), (4096, 300), (64, 20000)])
def test_same_bits_from_call_to_call_and_object_to_object_and_index_width(qn, m, n):
    pr, x, _ = SC.truth_at(m, n, 1.0)
    one, two = _obj(qn, pr), _obj(qn, pr, dtype=np.int64)
    try:
        a1, a2, b1 = one(x), one(x), two(x)
        assert a1.f() == a2.f() == b1.f() and a1.g().tobytes() == a2.g().tobytes() == b1.g().tobytes()
        (q1, c1), (q2, c2), (q3, c3) = one.hess_vec_at(x, pr["v"]), one.hess_vec_at(x, pr["v"]), two.hess_vec_at(x, pr["v"])
        assert c1 == c2 == c3 and q1.tobytes() == q2.tobytes() == q3.tobytes()
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
    pr, x, _ = SC.truth_at(96, 64, 1.0)
    base = _obj(qn, pr)
    coo = sp.coo_matrix(sp.csr_matrix((pr["data"], pr["indices"], pr["indptr"]), shape=(96, 64)))
    objs = [qn.SparseLogistic.from_scipy(coo, pr["y"], pr["mu"], weights=pr["w"]),
            qn.SparseLogistic(pr["indptr"].astype(np.int64), pr["indices"], pr["data"], pr["y"], pr["mu"], 64, weights=pr["w"]),  # a mixed pair
            qn.SparseLogistic(pr["indptr"].astype(np.uint16), pr["indices"].astype(np.uint16), pr["data"], pr["y"], pr["mu"], 64, weights=pr["w"])]
    try:
        ref = base(x)
        for o in objs:
            ev = o(x)
            assert ev.f() == ref.f() and ev.g().tobytes() == ref.g().tobytes()
    finally:
        for o in objs + [base]:
            o.close()


def test_the_dense_logistic_beside_it(qn):
    """hess_vec_at and the evaluation of the dense Logistic on the densified (96, 64) problem: both inside the bounds of the same truth"""
    pr, x, truth = SC.truth_at(96, 64, 1.0)
    sparse, dense = _obj(qn, pr), qn.Logistic(pr["a"], pr["y"], pr["mu"], weights=pr["w"])
    try:
        for name, obj in (("sparse", sparse), ("dense", dense)):
            ev = obj(x)
            q, c = obj.hess_vec_at(x, pr["v"])
            r = RL.ratios(dict(f=ev.f(), g=ev.g(), q=q, c=c), truth)
            assert max(r.values()) <= 1.0, (name, r)
    finally:
        sparse.close()
        dense.close()


# ---- 2. NewtonCG against the restatement, inside the licensed windows ----
def _ls(qn, kind):
    return qn.StrongWolfe(*SC.WOLFE) if kind == "wolfe" else qn.BackTracking(1e-4, 0.5)


def _bytes_model(pr):
    m, n = pr["a"].shape
    base = 24 * pr["data"].size + 4 * (m + 1) + 4 * (n + 1) + 24 * n
    return base + 32 * m, base + 24 * m  # (one evaluation, one product)


def newton_run(qn, m, n, ls, iters=SC.ITERS, memoize=1, chunk=8, mu=None, calls=1):
    pr = SC.problem(m, n)
    obj = _obj(qn, pr, mu)
    s = qn.NewtonCG(SC.TOL, pr["x0"], chunk=chunk, memoize=memoize)
    out = dict(trace=[], xs=[], inner=[], neg=[], fb=[], hv=0, inner_total=0, status="ok", k=0)
    try:
        for _ in range(calls):
            s.set_trace(iters, with_x=True)
            rec = []
            try:
                s.minimize(_ls(qn, ls), obj, iters, SC.MAX_LS, callback=lambda sv: rec.append((sv.inner_iterations()[0], sv.negative_curvature(), sv.fallbacks())))
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
@pytest.mark.parametrize("m,n,ls", SC.CASES)
def test_newton_cg_against_the_restatement(qn, m, n, ls, memoize):
    w = SC.window(m, n, ls)
    ref = SC.ref_case(m, n, ls)[0]
    run = _run(qn, m, n, ls, memoize, 8)
    assert len(run["trace"]) >= w and len(run["inner"]) == len(run["trace"])
    worst = 0.0
    for k in range(w):
        r, g = ref.trace[k], run["trace"][k]
        dx = float(np.linalg.norm(run["xs"][k] - ref.trace_x[k]) / max(1.0, np.linalg.norm(ref.trace_x[k])))
        worst = max(worst, dx)
        assert dx <= SC.GPU_TOL, (k, dx)
        assert g["n_evals"] == r["n_evals"] and g["ls_iters"] == r["ls_iters"], (k, g, r)
        assert (g["t"] == r["t"]) if ls == "bt" else (abs(g["t"] - r["t"]) <= SC.GPU_TOL * abs(r["t"])), (k, g["t"], r["t"])
        assert run["inner"][k] == ref.inner[k], (k, run["inner"], ref.inner)
    assert run["neg"][w - 1] == 0 and run["fb"][w - 1] == 0 and set(ref.why[:w]) <= {"tol", "cap"}
    if (m, n) in SC.CONVERGENCE:  # the convergence shapes reach 1e-7 in the restatement's iteration count, under both searches
        assert run["status"] == "ok" and SC.ref_case(m, n, ls)[2] == "ok" and run["k"] == ref.k, (run["k"], ref.k, run["status"])
    print(f"sparse logistic NewtonCG {(m, n, ls)} memoize={memoize}: window {w} of {len(ref.trace)}, worst |x - x_ref| = {worst:.2e}, GPU k = {run['k']} ({run['status']}), "
          f"inner {sum(run['inner'])}")


@pytest.mark.parametrize("m,n,ls", [(96, 64, "bt"), (257, 200, "wolfe"), (5, 2050, "bt"), (64, 20000, "bt")])
def test_the_chunk_never_changes_a_bit(qn, m, n, ls):
    base = _bits(_run(qn, m, n, ls, 1, 8))
    for chunk in (1, 3):
        assert _bits(_run(qn, m, n, ls, 1, chunk)) == base, chunk
    assert _bits(_run(qn, m, n, ls, 0, 8)) == base  # (memoize 0 evaluates the accepted point again: the same bits)


@pytest.mark.parametrize("m,n", SC.CONVERGENCE)
def test_convergence_and_one_weights_pass_per_iteration(qn, m, n):
    ref, _, ref_status = SC.ref_case(m, n, "bt")
    assert ref_status == "ok"
    run = _run(qn, m, n, "bt", 1, 8)
    assert run["status"] == "ok" and run["k"] == ref.k, (run["k"], ref.k)
    pr = SC.problem(m, n)
    g = RL.truth_and_bound(pr["a"], pr["y"], pr["w"], pr["mu"], run["x"])["g"]
    assert float(np.max(np.abs(g))) < SC.TOL
    assert run["hv"] == run["inner_total"] == sum(run["inner"])
    # obj_bytes = (evaluations + ONE weights pass per loop top) * an evaluation's bytes + products * a product's bytes, exactly: k outer iterations
    # and the loop top that found the run converged (the weights' launches are the unpredicated ones of a batch)
    eval_bytes, product_bytes = _bytes_model(pr)
    assert run["obj_bytes"] == (run["evals"] + run["k"] + 1) * eval_bytes + run["hv"] * product_bytes, (run["obj_bytes"], run["evals"], run["hv"], run["k"])
    assert run["path"] & qn._abi.PATH_NEWTON_CG and run["path"] & qn._abi.PATH_VECTOR
    print(f"sparse logistic NewtonCG {(m, n)} bt: outer {run['k']}, inner {run['inner_total']}, evaluations {run['evals']}, weights passes {run['k'] + 1}, launches {run['launches']}")


def test_negative_mu_takes_the_gradient(qn):
    ghg, gg = SC.neg_mu_curvature()
    assert ghg < 0.0 < gg  # chosen on the host: rule 4 at j = 0
    ref = SC.run_ref(3, 5, "bt", iters=3, mu=SC.NEG_MU)[0]
    assert ref.why[0] == "negcurv" and ref.inner[0] == 0
    run = newton_run(qn, 3, 5, "bt", iters=3, mu=SC.NEG_MU)
    assert run["neg"][0] >= 1 and run["inner"][0] == 0
    pr = SC.problem(3, 5)
    g0 = RL.logistic_fn(pr["a"], pr["y"], pr["w"], SC.NEG_MU)(pr["x0"])[1]
    t0 = run["trace"][0]["t"]
    assert np.linalg.norm(run["xs"][0] - (pr["x0"] + t0 * -g0)) <= SC.GPU_TOL * max(1.0, np.linalg.norm(pr["x0"]))  # d = -g
    for k in range(min(3, len(ref.trace), len(run["trace"]))):
        assert run["inner"][k] == ref.inner[k] and run["trace"][k]["t"] == ref.trace[k]["t"] and run["trace"][k]["n_evals"] == ref.trace[k]["n_evals"], k


def test_two_calls_are_one(qn):
    one = newton_run(qn, 96, 64, "bt", iters=8)
    two = newton_run(qn, 96, 64, "bt", iters=4, calls=2)
    assert one["x"].tobytes() == two["x"].tobytes() and one["inner"] == two["inner"]
    assert [x.tobytes() for x in one["xs"]] == [x.tobytes() for x in two["xs"]]


# ---- 3. the rest of the family: the existing restatements on logistic_fn of the densified matrix, and beside a host closure of it ----
def _family_gpu(qn, kind, m, n, oracle, iters):
    pr = SC.problem(m, n)
    x0 = pr["x0"]
    lb, ub = SC.family_box(kind, n)
    if kind == "lbfgs":
        s, ls = qn.LBFGS(SC.FAMILY_TOL, x0, m=5, memoize=1), qn.StrongWolfe()
    elif kind == "cg":
        s, ls = qn.NonlinearCG(SC.FAMILY_TOL, x0, variant="pr+", memoize=1), qn.StrongWolfe(1e-4, 0.1)
    elif kind == "spg":
        s, ls = qn.SpectralProjectedGradient(SC.FAMILY_TOL, x0, oracle, lb, ub, memoize=1), qn.GLLQuadratic(1e-4, 10)
    else:
        s, ls = qn.ProjectedLBFGS(SC.FAMILY_TOL, x0, lb, ub, m=5, memoize=1), qn.BackTrackingB(1e-4, 0.5, lb, ub)
    s.set_trace(iters, with_x=True)
    try:
        s.minimize(ls, oracle, iters, 50)
    except qn.MaxIterReached:
        pass
    return s


@pytest.mark.parametrize("kind,m,n", SC.FAMILY_CASES)
def test_the_rest_of_the_family(qn, kind, m, n):
    ref, w = SC.family_licence(kind, m, n)
    assert w >= 4
    pr = SC.problem(m, n)
    fn = RL.logistic_fn(pr["a"], pr["y"], pr["w"], pr["mu"])
    obj = _obj(qn, pr)
    dev = host = None
    try:
        dev = _family_gpu(qn, kind, m, n, obj, w)
        host = _family_gpu(qn, kind, m, n, lambda x: fn(x), w)
        ref_w = type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
        for run in (dev, host):  # test_gpu_logistic's comparison: test_gpu_spg._compare, then `updated` and s_norm for the methods that have them
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
        assert sd["obj_bytes"] == sd["oracle_evals"] * _bytes_model(pr)[0]
        # THREE launches per evaluation: with memoize = 1 on both, the host closure's run makes the same launches but the objective's own (a device
        # objective's launches are unpredicated: the batch whose loop top ends the run may enqueue one evaluation that nothing asked for)
        extra = sd["launches"] - sh["launches"]
        print(f"sparse logistic {kind} {(m, n)}: window {w}, launches device {sd['launches']} host {sh['launches']}, evaluations {sd['oracle_evals']}, closure calls {sh['oracle_calls']}")
        assert extra % 3 == 0 and extra // 3 - sd["oracle_evals"] in (0, 1), (extra, sd["oracle_evals"])
    finally:
        for run in (dev, host):
            if run is not None:
                run.close()
        obj.close()


# ---- 4. refusals: each ErrorInputParams with its message, before anything is launched ----
def test_creation_refusals(qn):
    pr = SC.problem(3, 5)
    ip, ix, da, y = pr["indptr"], pr["indices"], pr["data"], pr["y"]
    assert da.size >= 4 and np.diff(ip).max() >= 2
    for bad in (0.0, 2.0):
        yb = y.copy()
        yb[2] = bad
        with pytest.raises(qn.ErrorInputParams, match="2 y - 1"):
            qn.SparseLogistic(ip, ix, da, yb, 0.5, 5)
    for bad in (-1.0, float("nan"), float("inf")):
        w = np.ones(3)
        w[1] = bad
        with pytest.raises(qn.ErrorInputParams, match="negative or not finite"):
            qn.SparseLogistic(ip, ix, da, y, 0.5, 5, weights=w)
    with pytest.raises(qn.ErrorInputParams, match="mu must be finite"):
        qn.SparseLogistic(ip, ix, da, y, float("inf"), 5)
    i = int(np.argmax(np.diff(ip) >= 2))  # a row with two entries
    swapped = ix.copy()
    swapped[ip[i]], swapped[ip[i] + 1] = ix[ip[i] + 1], ix[ip[i]]
    with pytest.raises(qn.ErrorInputParams, match="strictly increasing"):
        qn.SparseLogistic(ip, swapped, da, y, 0.5, 5)
    dup = ix.copy()
    dup[ip[i] + 1] = ix[ip[i]]
    with pytest.raises(qn.ErrorInputParams, match="strictly increasing"):
        qn.SparseLogistic(ip, dup, da, y, 0.5, 5)
    with pytest.raises(qn.ErrorInputParams, match=r"outside \[0, n\)"):  # a column >= n
        qn.SparseLogistic(ip, ix, da, y, 0.5, int(ix.max()))
    neg = ix.copy()
    neg[0] = -1
    with pytest.raises(qn.ErrorInputParams, match=r"outside \[0, n\)"):
        qn.SparseLogistic(ip, neg, da, y, 0.5, 5)
    for bad_ip, message in ((ip + 1, r"row_ptr\[0\]"), (np.array([0, 1, 0, da.size], dtype=ip.dtype), "decreases"),
                            (np.concatenate([ip[:-1], [da.size - 1]]).astype(ip.dtype), r"row_ptr\[m\]")):
        with pytest.raises(qn.ErrorInputParams, match=message):
            qn.SparseLogistic(bad_ip, ix, da, y, 0.5, 5)
    with pytest.raises(qn.ErrorInputParams, match="do not match"):
        qn.SparseLogistic(ip[:-1], ix, da, y, 0.5, 5)
    with pytest.raises(qn.ErrorInputParams, match="empty shape"):
        qn.SparseLogistic(ip, ix, da, y, 0.5, 0)
    ok = qn.SparseLogistic(ip, ix, da, y, -3.0, 5)  # (any finite mu)
    ok.close()
    empty = qn.SparseLogistic(np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), y, 0.5, 5)  # nnz = 0: f = sum w log 2 + mu/2 ||x||^2
    try:
        ev = empty(pr["x0"])
        assert abs(ev.f() - (3.0 * np.log(2.0) + 0.25 * float(pr["x0"] @ pr["x0"]))) <= 1e-14 * ev.f() and np.array_equal(ev.g(), 0.5 * pr["x0"])
    finally:
        empty.close()


def test_a_two_rank_context_is_refused(qn):
    def gather(send, recv):
        recv[:send.size] = send
        recv[send.size:] = send
    ctx = qn.Context(0, 0, 2, host_allgather=gather)  # (world = 2 through the host exchange, this rank alone)
    try:
        with pytest.raises(qn.ErrorInputParams, match="single-GPU"):
            _obj(qn, SC.problem(3, 5), ctx=ctx)
    finally:
        ctx.close()


def test_solver_and_entry_point_refusals(qn):
    pr = SC.problem(3, 5)
    obj = _obj(qn, pr)
    quad = qn.Quadratic(np.eye(5), np.zeros(5))
    x0 = pr["x0"]
    try:
        lb, ub = np.full(5, -1.0), np.full(5, 1.0)
        # the dense quasi-Newton family, the control-step solvers and Newton, then the projected Newton pair: refused before anything is launched
        refused = [(qn.BFGS(1e-8, x0), "SparseLogistic"), (qn.DFP(1e-8, x0), "SparseLogistic"), (qn.Broyden(1e-8, x0), "SparseLogistic"),
                   (qn.GradientDescent(1e-8, x0), "SparseLogistic"), (qn.CoordinateDescent(1e-8, x0), "SparseLogistic"), (qn.Newton(1e-8, x0), "SparseLogistic"),
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
        with pytest.raises(qn.ErrorInputParams, match="no dense rows / Hessian"):
            obj.hessian(x0)
        with pytest.raises(qn.ErrorInputParams, match="hess_vec_at"):
            obj.hess_vec(x0)
        with pytest.raises(qn.ErrorInputParams, match="no dense rows / Hessian"):
            obj.rows(0, 1)
        with pytest.raises(qn.ErrorInputParams, match="qn_sparse_logistic_info"):
            qn.SparseQuadratic._info(obj)  # (qn_objective_sparse_info on this handle)
        with pytest.raises(qn.ErrorInputParams, match="not a sparse logistic"):
            qn.SparseLogistic._info(quad)
        tn = qn.NewtonCG(1e-7, x0)
        with pytest.raises(qn.ErrorInputParams, match="LogSumExp or Logistic"):
            tn.minimize(qn.BackTracking(1e-4, 0.5), quad, 5, 5)
        with pytest.raises(qn.ErrorInputParams, match="BackTracking or StrongWolfe"):
            tn.minimize(qn.GLLQuadratic(1e-4, 10), obj, 5, 5)
        tn.close()
        boxed = qn.NewtonCG(1e-7, x0)  # (a box under NewtonCG: out of scope, whatever the objective)
        with pytest.raises(qn.ErrorInputParams, match="unbounded only"):
            boxed.minimize(qn.StrongWolfe().with_lower_bound(lb), obj, 5, 5)
        boxed.close()
    finally:
        obj.close()
        quad.close()
