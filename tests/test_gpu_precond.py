"""GPU tests of the Hessian diagonal (Objective.hess_diag_at; kernels csrc/qn_hess_diag.hip.h and slog_diag_kernel in csrc/qn_sparse_logistic.hip.h)
and of NewtonCG's Jacobi preconditioner (csrc/qn_newton_cg.hip.h, rules 1' to 7'): the diagonal against np.longdouble inside the derived bounds of
tests/ref_newton_pcg.py, bit-for-bit repeatability, 1 / M and its floor, the refusals, the preconditioned runs against the restatement inside the
windows tests/test_ref_precond.py licenses, convergence in at most half the plain GPU run's inner steps, the counters, warm restarts, and
preconditioner="none" against a solver that never heard of the option.

MEASURED on one MI355X (the largest |error| / bound of the diagonal over all shapes, scales and lane counts, printed by the tests):
Logistic 0.987, LogSumExp 0.183, SparseLogistic 0.949 (the values near 1: (3, 16384) and (5, 2050) at scale 1e-3, the last addition's half ulp against
the bound's own term for it)."""
import math

import numpy as np
import pytest

import logistic_cases as LC
import lse_hess_vec_cases as HV
import precond_cases as PC
import ref_logistic as RL
import ref_newton_pcg as RP
import sparse_logistic_cases as SC

pytestmark = pytest.mark.gpu
_worst = {}

# (1, 1), (3, 5): workgroups that own no row; (40, 65), (257, 200): an uneven cut; KCH 2, 4, 16 with n_pad at its limit; 256 workgroups
DENSE_SHAPES = [(1, 1), (3, 5), (40, 65), (257, 200), (7, 1030), (5, 2050), (3, 16384), (1024, 1024)]


def _note(key, r):
    _worst[key] = max(_worst.get(key, 0.0), r)
    return r


def _sparse(qn, pr, mu=None, dtype=None, ctx=None):
    ip, ix = (pr["indptr"], pr["indices"]) if dtype is None else (pr["indptr"].astype(dtype), pr["indices"].astype(dtype))
    return qn.SparseLogistic(ip, ix, pr["data"], pr["y"], pr["mu"] if mu is None else mu, pr["a"].shape[1], weights=pr["w"], ctx=ctx)


# ---- 1. the diagonal against longdouble ----
@pytest.mark.parametrize("m,n", DENSE_SHAPES)
def test_logistic_diagonal_inside_its_bound(qn, m, n):
    """Logistic at logistic_cases' scales, the first and the last row of a workgroup's cut masked"""
    obj = None
    try:
        for scale in LC.SCALES:
            pr, x, truth = LC.truth_at(m, n, scale, "edges")
            a, y, w, mu = pr[:4]
            obj = obj or qn.Logistic(a, y, mu, weights=w)
            ms, bound = RP.logistic_diag_truth(a, y, w, mu, x, truth)
            r = _note("logistic", RP.ratio(obj.hess_diag_at(x), ms, bound))
            print(f"logistic diagonal {(m, n)} scale {scale:g}: max |M - M*| / bound = {r:.3f}")
            assert r <= 1.0, (scale, r)
    finally:
        if obj:
            obj.close()
    print("diagonal worst so far:", {k: f"{v:.3f}" for k, v in _worst.items()})


@pytest.mark.parametrize("m,n", DENSE_SHAPES[:5])
def test_lse_diagonal_inside_its_bound(qn, m, n):
    a, c, mu, x0, _ = HV.problem(m, n)
    obj = qn.LogSumExp(a, c, mu)
    try:
        for scale in HV.SCALES:
            ms, bound = RP.lse_diag_truth(a, c, mu, scale * x0)
            r = _note("lse", RP.ratio(obj.hess_diag_at(scale * x0), ms, bound))
            print(f"log-sum-exp diagonal {(m, n)} scale {scale:g}: max |M - M*| / bound = {r:.3f}")
            assert r <= 1.0, (scale, r)
    finally:
        obj.close()
    print("diagonal worst so far:", {k: f"{v:.3f}" for k, v in _worst.items()})


def test_lse_diagonal_with_a_masked_row(qn):
    m, n = HV.MASK_SHAPE
    for row in HV.MASK_ROWS.values():
        a, c, mu, x0, _ = HV.problem(m, n, row)
        obj = qn.LogSumExp(a, c, mu)
        try:
            ms, bound = RP.lse_diag_truth(a, c, mu, x0)
            assert _note("lse", RP.ratio(obj.hess_diag_at(x0), ms, bound)) <= 1.0
        finally:
            obj.close()


@pytest.mark.parametrize("m,n", SC.SHAPES)
def test_sparse_diagonal_inside_its_bound(qn, m, n):
    """sparse_logistic_cases.SHAPES: the empty column of (40, 65), the column of ones over 2050 rows (a long row of A'), (64, 20000)"""
    for kind in ("weighted", "edges"):
        obj = _sparse(qn, SC.problem(m, n, kind))
        try:
            for scale in SC.SCALES if kind == "weighted" else [1.0]:
                pr, x, truth = SC.truth_at(m, n, scale, kind)
                ms, bound = RP.logistic_diag_truth(pr["a"], pr["y"], pr["w"], pr["mu"], x, truth)
                got = obj.hess_diag_at(x)
                r = _note("sparse", RP.ratio(got, ms, bound))
                print(f"sparse logistic diagonal {(m, n)} {kind} scale {scale:g}: max |M - M*| / bound = {r:.3f}")
                assert r <= 1.0, (kind, scale, r)
                if (m, n) == (40, 65):
                    assert got[64] == pr["mu"]  # the empty column: M_j = mu exactly
        finally:
            obj.close()
    print("diagonal worst so far:", {k: f"{v:.3f}" for k, v in _worst.items()})


def test_every_lane_count_on_the_column_pass(qn):
    pr, x, truth = SC.truth_at(40, 65, 1.0)
    ms, bound = RP.logistic_diag_truth(pr["a"], pr["y"], pr["w"], pr["mu"], x, truth)
    obj = _sparse(qn, pr)
    try:
        base = obj.hess_diag_at(x)
        for lanes in SC.LANES:
            obj.set_lanes(1, lanes)
            got = obj.hess_diag_at(x)
            assert _note("sparse", RP.ratio(got, ms, bound)) <= 1.0 and got[64] == pr["mu"], lanes
        obj.set_lanes(0, 0)
        assert obj.hess_diag_at(x).tobytes() == base.tobytes()
    finally:
        obj.close()


# ---- 2. determinism ----
def test_same_bits_from_call_to_call_object_to_object_and_index_width(qn):
    for (m, n) in [(257, 200), (5, 2050), (1024, 1024)]:
        pr, x, _ = LC.truth_at(m, n, 1.0, "edges")
        one, two = qn.Logistic(pr[0], pr[1], pr[3], weights=pr[2]), qn.Logistic(pr[0].copy(), pr[1].copy(), pr[3], weights=pr[2].copy())
        try:
            a1 = one.hess_diag_at(x)
            one(30.0 * x)  # (an evaluation elsewhere: the diagonal forms its own weights at x)
            assert a1.tobytes() == one.hess_diag_at(x).tobytes() == two.hess_diag_at(x).tobytes()
        finally:
            one.close()
            two.close()
    a, c, mu, x0, _ = HV.problem(257, 200)
    one, two = qn.LogSumExp(a, c, mu), qn.LogSumExp(a.copy(), c.copy(), mu)
    try:
        a1 = one.hess_diag_at(x0)
        assert a1.tobytes() == one.hess_diag_at(x0).tobytes() == two.hess_diag_at(x0).tobytes()
    finally:
        one.close()
        two.close()
    for (m, n) in [(96, 64), (2050, 7), (4096, 300), (64, 20000)]:
        pr, x, _ = SC.truth_at(m, n, 1.0)
        one, two = _sparse(qn, pr), _sparse(qn, pr, dtype=np.int64)
        try:
            a1 = one.hess_diag_at(x)
            assert a1.tobytes() == one.hess_diag_at(x).tobytes() == two.hess_diag_at(x).tobytes()
        finally:
            one.close()
            two.close()


# ---- 3. refusals, before any launch ----
def test_refusals(qn):
    rng = np.random.default_rng(11)
    wide = qn.LogSumExp(rng.standard_normal((2, LC.TOO_WIDE)), np.zeros(2), 0.1)
    try:
        with pytest.raises(qn.ErrorInputParams, match="not built"):
            wide.hess_diag_at(np.zeros(LC.TOO_WIDE))
        s = qn.NewtonCG(1e-7, np.zeros(LC.TOO_WIDE), preconditioner="jacobi")
        try:
            with pytest.raises(qn.ErrorInputParams, match="not built"):
                s.minimize(qn.BackTracking(1e-4, 0.5), wide, 3, 5)
            assert s.stats()["launches"] == 0
        finally:
            s.close()
    finally:
        wide.close()
    a = rng.standard_normal((6, 4))
    q = a.T @ a + np.eye(4)
    ip, ix, data = SC.to_csr(q, np.ones((4, 4), dtype=bool))
    lab = np.array([0, 1, 2, 0, 1, 2])
    aip, aix, adata = SC.to_csr(a, np.ones((6, 4), dtype=bool))
    others = [qn.Multinomial(a, lab, 3, 0.5), qn.SparseMultinomial(aip, aix, adata, lab, 3, 0.5, 4),
              qn.Quadratic(q, np.ones(4)), qn.SparseQuadratic(ip, ix, data, np.ones(4))]
    try:
        for obj in others:
            with pytest.raises(qn.ErrorInputParams, match="not built for this objective"):
                obj.hess_diag_at(np.zeros(obj.n))
        for obj in others[:2]:  # (a quadratic is refused by NewtonCG itself, with or without a preconditioner)
            s = qn.NewtonCG(1e-7, np.zeros(obj.n), preconditioner="jacobi")
            try:
                with pytest.raises(qn.ErrorInputParams, match="needs an objective with a Hessian diagonal"):
                    s.minimize(qn.BackTracking(1e-4, 0.5), obj, 3, 5)
                assert s.stats()["launches"] == 0
                s.set_preconditioner("none")  # the same solver runs once the option is off
                try:
                    s.minimize(qn.BackTracking(1e-4, 0.5), obj, 2, 5)
                except qn.MaxIterReached:
                    pass
                assert s.diag_passes() == 0
            finally:
                s.close()
    finally:
        for obj in others:
            obj.close()
    s = qn.NewtonCG(1e-7, np.zeros(4))
    try:
        assert s.preconditioner == "none"
        with pytest.raises(qn.ErrorInputParams, match='"none" or "jacobi"'):
            s.set_preconditioner("ssor")
        assert qn._abi.lib().qn_solver_set_newton_cg_preconditioner(s.h, 2) == qn._abi.ERROR_INPUT_PARAMS
        with pytest.raises(qn.ErrorInputParams, match="no run with the Jacobi"):
            s.preconditioner_diag()
        s.set_preconditioner("jacobi")
        assert s.preconditioner == "jacobi"
    finally:
        s.close()
    other = qn.LBFGS(1e-7, np.zeros(4))
    try:
        assert qn._abi.lib().qn_solver_set_newton_cg_preconditioner(other.h, 1) == qn._abi.ERROR_INPUT_PARAMS
        assert b"NewtonCG" in qn._abi.lib().qn_last_error_message()
    finally:
        other.close()
    with pytest.raises(qn.ErrorInputParams, match='"none" or "jacobi"'):
        qn.NewtonCG(1e-7, np.zeros(4), preconditioner="diag")


def test_a_row_sharded_context_is_refused(qn):
    def gather(send, recv):
        recv[:send.size] = send
        recv[send.size:] = send
    ctx = qn.Context(0, 0, 2, host_allgather=gather)  # (world = 2 through the host exchange, this rank alone)
    try:
        rng = np.random.default_rng(5)
        obj = qn.LogSumExp(rng.standard_normal((32, 6)), rng.standard_normal(32), 0.1, ctx=ctx)
        try:
            with pytest.raises(qn.ErrorInputParams, match="single-GPU"):
                obj.hess_diag_at(np.zeros(6))
        finally:
            obj.close()
    finally:
        ctx.close()


# ---- 4. the preconditioned runs ----
def _objective(qn, kind, pr, mu=None):
    mu = pr["mu"] if mu is None else mu
    return _sparse(qn, pr, mu) if kind == "sparse" else qn.Logistic(pr["a"], pr["y"], mu, weights=pr["w"])


def newton_run(qn, kind, pr, ls, precond, iters=PC.ITERS, chunk=8, calls=1, mu=None, default_solver=False):
    obj = _objective(qn, kind, pr, mu)
    s = qn.NewtonCG(PC.TOL, pr["x0"], chunk=chunk) if default_solver else qn.NewtonCG(PC.TOL, pr["x0"], chunk=chunk, preconditioner=precond)
    out = dict(trace=[], xs=[], inner=[], neg=[], fb=[], hv=0, inner_total=0, diag=0, status="ok", k=0, syncs=0)
    try:
        for _ in range(calls):
            s.set_trace(iters, with_x=True)
            rec = []
            try:
                s.minimize(qn.StrongWolfe(*PC.WOLFE) if ls == "wolfe" else qn.BackTracking(1e-4, 0.5), obj, iters, PC.MAX_LS,
                           callback=lambda sv: rec.append((sv.inner_iterations()[0], sv.negative_curvature(), sv.fallbacks())))
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
            out["diag"] += s.diag_passes()
            out["k"] += s.k()
            out["syncs"] += st["host_syncs"]
            out["obj_bytes"], out["evals"], out["launches"] = st["obj_bytes"], st["oracle_evals"], st["launches"]
        out["x"] = s.x()
        out["floored"] = s.diag_floored()
        out["pc"] = s.preconditioner_diag() if s.preconditioner == "jacobi" else None
    finally:
        s.close()
        obj.close()
    return out


def _bits(run):
    return (run["x"].tobytes(), [x.tobytes() for x in run["xs"]], [(r["t"], r["n_evals"], r["f"]) for r in run["trace"]], run["inner"], run["status"])


_runs = {}


def _run(qn, kind, m, n, ls, precond):
    key = (kind, m, n, ls, precond)
    if key not in _runs:
        _runs[key] = newton_run(qn, kind, PC.problem(m, n, kind), ls, precond)
    return _runs[key]


@pytest.mark.parametrize("kind,m,n,ls", PC.CASES)
def test_jacobi_against_the_restatement(qn, kind, m, n, ls):
    """every decision of the restatement inside its window: t, n_evals, the inner count, the exit reason (a loop that ended by the tolerance or the
    cap: no negative curvature, no fallback); x within GPU_TOL"""
    w = PC.window(kind, m, n, ls)
    ref = PC.ref_case(kind, m, n, ls)[0]
    run = _run(qn, kind, m, n, ls, "jacobi")
    assert len(run["trace"]) >= w and len(run["inner"]) == len(run["trace"])
    worst = 0.0
    for k in range(w):
        r, g = ref.trace[k], run["trace"][k]
        dx = float(np.linalg.norm(run["xs"][k] - ref.trace_x[k]) / max(1.0, np.linalg.norm(ref.trace_x[k])))
        worst = max(worst, dx)
        assert dx <= PC.GPU_TOL, (k, dx)
        assert g["n_evals"] == r["n_evals"] and g["ls_iters"] == r["ls_iters"], (k, g, r)
        assert (g["t"] == r["t"]) if ls == "bt" else (abs(g["t"] - r["t"]) <= PC.GPU_TOL * abs(r["t"])), (k, g["t"], r["t"])
        assert run["inner"][k] == ref.inner[k], (k, run["inner"], ref.inner)
    assert run["neg"][w - 1] == 0 and run["fb"][w - 1] == 0 and set(ref.why[:w]) <= {"tol", "cap"}
    print(f"Jacobi NewtonCG {(kind, m, n, ls)}: window {w} of {len(ref.trace)}, worst |x - x_ref| = {worst:.2e}, GPU k = {run['k']} ({run['status']})")


@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("m,n", PC.SHAPES)
def test_convergence_in_at_most_half_the_inner_steps_and_the_counters(qn, kind, m, n):
    """against the existing path on the same problem, not a stored number"""
    pr = PC.problem(m, n, kind)
    run, plain = _run(qn, kind, m, n, "bt", "jacobi"), _run(qn, kind, m, n, "bt", "none")
    assert run["status"] == "ok" and plain["status"] == "ok"
    g = RL.truth_and_bound(pr["a"], pr["y"], pr["w"], pr["mu"], run["x"])["g"]
    assert float(np.max(np.abs(g))) < PC.TOL
    print(f"precond {kind} {(m, n)}: plain {plain['k']} outer / {plain['inner_total']} inner; Jacobi {run['k']} / {run['inner_total']}; "
          f"host_syncs {plain['syncs']} / {run['syncs']}")
    assert run["inner_total"] <= PC.HALF * plain["inner_total"], (run["inner_total"], plain["inner_total"])
    # the counters: one diagonal per direction started; no entry floored (every M_j >= mu > 0)
    assert run["diag"] == run["k"] == len(run["inner"]) and run["floored"] == 0 and plain["diag"] == 0
    assert run["hv"] == run["inner_total"] == sum(run["inner"])
    # obj_bytes: evaluations, products, and ONE weights pass and ONE diagonal pass per loop top (k iterations and the loop top that found the run
    # converged: the unpredicated launches of a batch)
    tops = run["k"] + 1
    if kind == "dense":
        stream = 8 * m * 16 * ((n + 15) // 16)
        assert run["obj_bytes"] == (run["evals"] + run["hv"] + 2 * tops) * stream
        assert plain["obj_bytes"] == (plain["evals"] + plain["hv"] + plain["k"] + 1) * stream
    else:
        nnz = pr["data"].size
        ev = 24 * nnz + 4 * (m + 1) + 4 * (n + 1) + 32 * m + 24 * n
        prod = 24 * nnz + 4 * (m + 1) + 4 * (n + 1) + 24 * m + 24 * n
        diag = 12 * nnz + 4 * (n + 1) + 8 * m + 16 * n
        assert run["obj_bytes"] == (run["evals"] + tops) * ev + run["hv"] * prod + tops * diag
    # host_syncs: the existing bound (tests/test_gpu_newton_cg.py) -- the diagonal pass adds no host read
    extra_trials = sum(r["ls_iters"] - 1 for r in run["trace"])
    budget = sum(max(1, math.ceil(j / 8)) for j in run["inner"]) + extra_trials + 2
    assert run["syncs"] <= budget, (run["syncs"], budget)


@pytest.mark.parametrize("kind", PC.KINDS)
def test_minv_is_one_over_m_bit_for_bit(qn, kind):
    m, n = 96, 64
    pr = PC.problem(m, n, kind)
    run = newton_run(qn, kind, pr, "bt", "jacobi", iters=3)
    mdiag, minv = run["pc"]
    assert np.all(mdiag > 0.0) and minv.tobytes() == (1.0 / mdiag).tobytes() and run["floored"] == 0
    # the solver's M is the public diagonal at the point of the last loop top (the diagonal pass is unpredicated: the loop top that ends a run
    # at its cap may or may not have enqueued one more): the same launches, the same bits
    obj = _objective(qn, kind, pr)
    try:
        assert mdiag.tobytes() in (obj.hess_diag_at(run["xs"][2]).tobytes(), obj.hess_diag_at(run["xs"][1]).tobytes())
    finally:
        obj.close()


@pytest.mark.parametrize("kind", PC.KINDS)
def test_negative_mu_floors_every_entry_and_the_launch_model(qn, kind):
    """mu = NEG_MU on (3, 5): every M_j <= 0 is floored, minv = 1, so the preconditioned run IS the plain run bit for bit -- and what it adds to
    stats.launches and obj_bytes is exactly the documented model: the diagonal's launches and bytes once per loop top, no host read more"""
    pr = (lambda p: dict(a=p[0], y=p[1], w=p[2], mu=p[3], x0=p[4]))(LC.problem(3, 5)) if kind == "dense" else SC.problem(3, 5)
    plain = newton_run(qn, kind, pr, "bt", "none", iters=3, mu=LC.NEG_MU)
    run = newton_run(qn, kind, pr, "bt", "jacobi", iters=3, mu=LC.NEG_MU)
    mdiag, minv = run["pc"]
    assert np.all(mdiag <= 0.0) and np.all(minv == 1.0) and run["floored"] == 5
    assert run["neg"][0] >= 1 and run["inner"][0] == 0  # rule 4 at j = 0, as without the preconditioner
    assert _bits(run) == _bits(plain)
    tops = run["k"]  # (the loop top that ends the run at its cap may enqueue one pass more: unpredicated launches)
    launches, bytes_ = (2, 8 * 3 * 16) if kind == "dense" else (1, 12 * pr["data"].size + 4 * 6 + 8 * 3 + 16 * 5)
    extra = run["launches"] - plain["launches"]
    assert extra % launches == 0 and extra // launches in (tops, tops + 1), (extra, tops)
    assert run["obj_bytes"] - plain["obj_bytes"] == (extra // launches) * bytes_
    assert run["syncs"] == plain["syncs"] and run["diag"] == run["k"]


@pytest.mark.parametrize("kind", PC.KINDS)
def test_two_calls_are_one(qn, kind):
    pr = PC.problem(96, 64, kind)
    one = newton_run(qn, kind, pr, "bt", "jacobi", iters=8)
    two = newton_run(qn, kind, pr, "bt", "jacobi", iters=4, calls=2)
    assert one["x"].tobytes() == two["x"].tobytes() and one["inner"] == two["inner"] and one["diag"] == two["diag"] == 8
    assert [x.tobytes() for x in one["xs"]] == [x.tobytes() for x in two["xs"]]


@pytest.mark.parametrize("ls", PC.SEARCHES)
def test_the_chunk_never_changes_a_bit(qn, ls):
    base = _bits(_run(qn, "dense", 96, 64, ls, "jacobi"))
    for chunk in (1, 3):
        assert _bits(newton_run(qn, "dense", PC.problem(96, 64), ls, "jacobi", chunk=chunk)) == base, chunk


def test_lse_with_the_preconditioner(qn):
    """log-sum-exp (gbar is not zero): the run follows the restatement on newton_cg_cases' (96, 64) problem for MIN_WINDOW iterations"""
    import newton_cg_cases as NC
    import ref_newton_cg as RN
    import ref_spg as R
    import spg_cases as S
    a, c, mu, x0 = NC.problem(96, 64)
    ref = RP.JacobiNewtonCG(NC.TOL, x0, RN.lse_hess_vec_at(a, c, mu), RP.lse_diag_at(a, c, mu))
    try:
        ref.minimize(R.BackTracking(1e-4, 0.5), R.CountingOracle(S.lse_fn(a, c, mu)), NC.MIN_WINDOW, NC.MAX_LS)
    except R.MaxIterReached:
        pass
    obj = qn.LogSumExp(a, c, mu)
    s = qn.NewtonCG(NC.TOL, x0, preconditioner="jacobi")
    try:
        s.set_trace(NC.MIN_WINDOW, with_x=True)
        inner = []
        try:
            s.minimize(qn.BackTracking(1e-4, 0.5), obj, NC.MIN_WINDOW, NC.MAX_LS, callback=lambda sv: inner.append(sv.inner_iterations()[0]))
        except qn.MaxIterReached:
            pass
        tr, xs = s.trace()
        w = min(len(ref.trace), len(tr))
        assert w >= 3 and s.diag_passes() == len(tr) and s.diag_floored() == 0
        for k in range(w):
            assert tr[k]["t"] == ref.trace[k]["t"] and tr[k]["n_evals"] == ref.trace[k]["n_evals"] and inner[k] == ref.inner[k], k
            assert np.linalg.norm(np.array(xs[k]) - ref.trace_x[k]) <= NC.GPU_TOL * max(1.0, np.linalg.norm(ref.trace_x[k])), k
        mdiag, minv = s.preconditioner_diag()
        assert minv.tobytes() == (1.0 / mdiag).tobytes()
    finally:
        s.close()
        obj.close()


# ---- 5. the existing path ----
def test_none_is_the_solver_that_never_heard_of_the_option(qn):
    """an existing case (logistic_cases (96, 64), BackTracking): preconditioner="none", and a solver switched to Jacobi and back, give the bits,
    the launches and the counters of a solver built without the keyword"""
    p = LC.problem(96, 64)
    pr = dict(a=p[0], y=p[1], w=p[2], mu=p[3], x0=p[4])
    base = newton_run(qn, "dense", pr, "bt", None, iters=LC.ITERS, default_solver=True)
    none = newton_run(qn, "dense", pr, "bt", "none", iters=LC.ITERS)
    assert _bits(none) == _bits(base)
    for key in ("launches", "obj_bytes", "evals", "syncs", "hv", "diag"):
        assert none[key] == base[key], key
    assert base["diag"] == 0
    obj = _objective(qn, "dense", pr)
    s = qn.NewtonCG(PC.TOL, pr["x0"], preconditioner="jacobi")
    try:
        s.set_preconditioner("none")
        s.set_trace(LC.ITERS, with_x=True)
        s.minimize(qn.BackTracking(1e-4, 0.5), obj, LC.ITERS, LC.MAX_LS)
        assert s.x().tobytes() == base["x"].tobytes() and s.stats()["launches"] == base["launches"] and s.diag_passes() == 0
    finally:
        s.close()
        obj.close()
