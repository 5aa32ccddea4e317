"""GPU tests of the ExactQuadratic line search (QN_LS_EXACT_QUADRATIC; kernels csrc/qn_vec_exact.hip.h and spq_curv_kernel of csrc/qn_sparse.hip.h) on the
four O(n) methods -- ProjectedGradientDescent, SpectralProjectedGradient, LBFGS / ProjectedLBFGS, NonlinearCG -- against the restatement tests/ref_exact.py
on the problems of tests/exact_cases.py.  Windows are licensed case by case by tests/test_ref_exact.py; the tolerance inside them is the family's,
1e-9 max(1, ||x||).  (The curvature pass on its own, against extended precision: tests/test_gpu_hess_vec.py.)"""
import os
import subprocess

import numpy as np
import pytest

import exact_cases as EC
import lbfgs_cases as LC
import sparse_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH_VECTOR, PATH_EXACT = 64, 4096
U = 2.0 ** -53


def _objective(qn, name, n, b=None):
    b = SC.rhs(n) if b is None else b
    if name == "dense":
        return qn.Quadratic(SC.dense(SC.tri(n)), b)
    return qn.SparseQuadratic(*EC.matrix(name, n), b)


def _solver(qn, method, name, n, obj, memoize=None, tol=EC.TOL, x0=None):
    x0 = SC.start(n) if x0 is None else x0
    lb, ub = EC.box_of(method, name, n)
    if method in ("pgd", "pgd-box"):
        s = qn.ProjectedGradientDescent(tol, x0, lb, ub)
        s.memoize = memoize
        return s
    if method in ("spg", "spg-box"):
        return qn.SpectralProjectedGradient(tol, x0, obj, lb, ub, memoize=memoize)
    if method in ("lbfgs", "plbfgs"):
        return qn.ProjectedLBFGS(tol, x0, lb, ub, m=EC.LBFGS_M, memoize=memoize)
    return qn.NonlinearCG(tol, x0, variant=method[3:], memoize=memoize)


def _run(qn, s, obj, r, iters, trace=True):
    if trace:
        s.set_trace(max(iters, 1), with_x=True)
    try:
        s.minimize(qn.ExactQuadratic(r), obj, iters, 0)
        return "ok"
    except qn.MaxIterReached:
        return "max_iter"
    except qn.AbnormalTermination as e:
        return "not_descent" if "not a descent direction" in str(e) else ("curvature" if "non-positive curvature" in str(e) else f"abnormal: {e}")


def _sparse_bytes(obj, n, evals, passes):
    return evals * (12 * obj.nnz + 4 * (n + 1) + 24 * n) + passes * (12 * obj.nnz + 4 * (n + 1) + 16 * n)


# ---- 1. the step itself ----
@pytest.mark.parametrize("n", [2, 7, 4099, (1 << 21) + 3])
def test_the_step_itself(qn, n):
    """one iteration of NonlinearCG (first direction exactly -g_0): the traced t against -(g.d) / (d.q) in extended precision, from the run's own g_0 and
    q.  Each sum is moved to both ends of +-(n + 1) u sum |a_i b_i| (any order of n products and n - 1 additions: gamma_n <= (n + 1) u; the reference's
    own 2^-64 is added), the quotient is taken at the four corners, and 4 u of the result covers the one division (the negation is exact)."""
    csr, b, x0 = SC.tri(n), SC.rhs(n), SC.start(n)
    obj, twin = qn.SparseQuadratic(*csr, b), qn.SparseQuadratic(csr[0].copy(), csr[1].copy(), csr[2].copy(), b.copy())
    try:
        g0 = obj(x0).g()
        d = -g0
        q, c = obj.hess_vec(d)
        q2, c2 = twin.hess_vec(-twin(x0).g())
        assert q.tobytes() == q2.tobytes() and np.float64(c).tobytes() == np.float64(c2).tobytes()  # the run's own bits, by determinism
        s = qn.NonlinearCG(0.0, x0, variant="fr")
        assert _run(qn, s, obj, 1, 1) == "max_iter"
        tr, xs = s.trace()
        t = tr[0]["t"]
        ld = np.longdouble
        num, den = np.sum(g0.astype(ld) * d.astype(ld)), np.sum(d.astype(ld) * q.astype(ld))
        e_num = (n + 1) * (U + 2.0 ** -64) * float(np.sum(np.abs(g0 * d)))
        e_den = (n + 1) * (U + 2.0 ** -64) * float(np.sum(np.abs(d * q)))
        assert abs(float(den)) > 4.0 * e_den
        corners = [float(-(num + sn * e_num) / (den + sd * e_den)) for sn in (-1, 1) for sd in (-1, 1)]
        lo, hi = min(corners), max(corners)
        slack = 4.0 * U * max(abs(lo), abs(hi))
        print(f"step n={n}: t={t!r} in [{lo!r}, {hi!r}] +- {slack:.2e}; width {(hi - lo) / abs(t):.2e} relative")
        assert lo - slack <= t <= hi + slack, (t, lo, hi)
        assert s.exact_state()["last_t"] == t and s.exact_state()["last_curvature"] == c
        assert np.array_equal(xs[0], x0 + t * d)
    finally:
        obj.close()
        twin.close()


# ---- 2. parity windows ----
@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_parity_window(qn, case):
    method, name, n, r = case
    ref, rls, ro, rstatus = EC.ref_case(case)
    w, whole_run, _ = EC.licence(case)
    iters = EC.WINDOW if whole_run else w
    obj = _objective(qn, name, n)
    try:
        runs = []
        for memoize in (0, 1):
            s = _solver(qn, method, name, n, obj, memoize=memoize)
            status = _run(qn, s, obj, r, iters)
            tr, xs = s.trace()
            st, ex = s.stats(), s.exact_state()
            assert st["path"] & PATH_VECTOR and st["path"] & PATH_EXACT
            if whole_run:
                assert status == rstatus == "ok" and len(tr) == len(ref.trace), (status, len(tr), len(ref.trace))
            else:
                assert len(tr) == w, (status, len(tr), w)
            for k in range(min(w, len(tr))):
                rk = ref.trace[k]
                assert abs(tr[k]["t"] - rk["t"]) <= 1e-9 * abs(rk["t"]), (k, tr[k]["t"], rk["t"])
                assert np.linalg.norm(xs[k] - ref.trace_x[k]) <= 1e-9 * max(1.0, np.linalg.norm(ref.trace_x[k])), k
                assert abs(tr[k]["gnorm"] - rk["gnorm"]) <= 1e-7 * max(1.0, rk["gnorm"]), k
                if rls.history[k]["capped"]:
                    assert tr[k]["t"] == 1.0, k
                if method.startswith("cg") or method in ("lbfgs", "plbfgs"):
                    assert tr[k]["updated"] == ref.updated[k], (k, tr[k]["updated"], ref.updated[k])  # CG: the restart pattern; L-BFGS: the commits
            if method.startswith("cg") and not whole_run:
                assert abs(s.beta() - ref.betas[w - 1]) <= 1e-9 * max(1.0, abs(ref.betas[w - 1]))
            assert ex["curvature_passes"] == st["iterations"] == len(tr)
            if not whole_run:  # (the run stopped at the window's end, where the restatement's counters are not: the rule, from the device's own numbers)
                if r == 1:
                    assert ex["refreshes"] == len(tr)
                if r == 3:
                    assert ex["refreshes"] >= len(tr) // 3
            # (SPG's CONSTRUCTOR evaluates x0 for lambda0 before any search is known, and keeps that evaluation only for a memoised oracle: with
            # memoize = 0 the first search's batch evaluates x0 again -- one evaluation and two launches more, the same bits)
            counts = () if method.startswith("spg") else (st["oracle_evals"], st["launches"])
            runs.append((xs.tobytes(), [x["t"] for x in tr], [x["f"] for x in tr], ex["refreshes"]) + counts)
        assert runs[0] == runs[1]  # memoize 0 and 1: the same bits, the same launches
    finally:
        obj.close()


# ---- 3. the budget ----
@pytest.mark.parametrize("name", ["tri", "dense"])
@pytest.mark.parametrize("method", ["cg-fr", "lbfgs", "pgd"])
def test_budget(qn, method, name):
    n, iters = 2050, 12
    obj = _objective(qn, name, n)
    dense_per_pass = set()
    try:
        for r in (0, 1, 3):
            s = _solver(qn, method, name, n, obj)
            assert _run(qn, s, obj, r, iters, trace=False) == "max_iter"
            st, ex = s.stats(), s.exact_state()
            it = st["iterations"]
            assert it == iters and ex["curvature_passes"] == it
            if r == 0:
                assert st["oracle_evals"] == 1 + ex["refreshes"]  # (every refresh is a forced one)
            if r == 1:
                assert st["oracle_evals"] == it + 1 and ex["refreshes"] == it
            if r == 3:
                assert ex["refreshes"] >= it // 3 and st["oracle_evals"] == 1 + ex["refreshes"]
            forced = ex["refreshes"] - (it if r == 1 else it // 3 if r == 3 else 0)
            assert 0 <= forced and st["host_syncs"] <= it + forced + 2, (st["host_syncs"], it, forced)
            if name == "tri":
                assert st["obj_bytes"] == _sparse_bytes(obj, n, st["oracle_evals"], it)
            else:  # the dense model: the padded matrix once per evaluation and once per curvature pass
                assert st["obj_bytes"] % (st["oracle_evals"] + it) == 0
                dense_per_pass.add(st["obj_bytes"] // (st["oracle_evals"] + it))
        if name == "dense":
            assert len(dense_per_pass) == 1 and min(dense_per_pass) >= 8 * n * n
    finally:
        obj.close()


# ---- 4. the point of the feature ----
def test_linear_cg_on_the_laplacian(qn):
    m = 64
    n = m * m
    csr, b = EC.laplacian(m), EC.laplacian_rhs(n)
    obj = qn.SparseQuadratic(*csr, b)
    try:
        s = qn.NonlinearCG(1e-8, np.zeros(n), variant="fr")
        assert _run(qn, s, obj, 0, 2000, trace=False) == "ok"  # QN_OK: a converged run
        x = s.x()
        ld = np.longdouble
        rows = SC.row_index(csr[0])
        qx = np.zeros(n, dtype=ld)
        np.add.at(qx, rows, csr[2].astype(ld) * x.astype(ld)[csr[1]])
        res = float(np.max(np.abs(qx - b.astype(ld))))
        counts = [EC.laplacian_cg(order)[0] for order in EC.ORDERS]
        margin = max(counts) - min(counts) + 2
        it, ex = s.stats()["iterations"], s.exact_state()
        print(f"laplacian {m} x {m}: GPU {it} iterations, restatement {counts} (margin {margin}); ||Qx - b||_inf = {res:.3e}; {ex}")
        assert res < 1e-8
        assert min(counts) - margin <= it <= max(counts) + margin
        assert ex["refreshes"] >= 1 and ex["curvature_passes"] == it  # a true gradient ended the run
        assert s.stats()["oracle_evals"] == 1 + ex["refreshes"]
    finally:
        obj.close()


# ---- 5. convergence is declared only on a true gradient ----
def test_convergence_confirmation(qn):
    method, name, n, r = EC.CONFIRM_CASE
    obj = _objective(qn, name, n)
    try:
        s = _solver(qn, method, name, n, obj, tol=EC.CONFIRM_TOL)
        status = _run(qn, s, obj, r, EC.CONFIRM_CAP, trace=False)
        it, ex = s.stats()["iterations"], s.exact_state()
        ref, _, ro, rstatus = EC.confirm_ref()
        print(f"confirmation: GPU {status} after {it} iterations, {ex['refreshes']} forced; restatement {rstatus} after {len(ref.trace)}, {ro.forced} forced; "
              f"the recurrence gradient first passes at iteration {EC.CONFIRM_FIRST_PASS}")
        assert status in ("ok", "max_iter")
        assert ex["refreshes"] >= 1          # the loop top's test passed on a recurrence gradient and the objective was asked
        assert it > EC.CONFIRM_FIRST_PASS    # ... and the run went on
        assert s.stats()["oracle_evals"] == 1 + ex["refreshes"]
    finally:
        obj.close()


# ---- 6. error paths ----
def test_rejected_oracles_methods_and_settings(qn):
    n = 7
    obj, dense = _objective(qn, "tri", n), _objective(qn, "dense", n)
    rng = np.random.default_rng(3)
    lse = qn.LogSumExp(rng.standard_normal((5, n)), rng.standard_normal(5), 0.1)
    x0 = SC.start(n)
    lb, ub = LC.free_box(n)
    try:
        fn = SC.quadratic_fn(SC.tri(n), SC.rhs(n))
        from test_gpu_device_closure import _Chain
        chain = _Chain(qn, np.ones(n), 0.3)
        for oracle in (fn, chain.closure, lse):  # a host closure, a device closure, log-sum-exp
            with pytest.raises(qn.ErrorInputParams, match="the exact step needs a device quadratic"):
                qn.NonlinearCG(1e-8, x0).minimize(qn.ExactQuadratic(1), oracle, 5, 0)
        for make in (lambda: qn.BFGS(1e-8, x0), lambda: qn.GradientDescent(1e-8, x0), lambda: qn.Newton(1e-8, x0),
                     lambda: qn.ProjectedNewton(1e-8, x0, lb, ub), lambda: qn.SpectralProjectedNewton(1e-8, x0, dense, lb, ub)):
            solver = make()  # (the dense quadratic: the Newton solvers' own checks want a Hessian, and this search must be refused before them)
            with pytest.raises(qn.ErrorInputParams, match="ExactQuadratic"):
                solver.minimize(qn.ExactQuadratic(1), dense, 5, 0)
        with pytest.raises(qn.ErrorInputParams, match="compute_step_len"):
            g0 = obj(x0)
            qn.ExactQuadratic(1).compute_step_len(x0, g0, -g0.g(), obj, 5)
        boxed = qn.ExactQuadratic(1)
        keep = np.full(n, -1.0)
        boxed.s.lower_bound_host = keep.ctypes.data
        with pytest.raises(qn.ErrorInputParams, match="no box of its own"):
            qn.NonlinearCG(1e-8, x0).minimize(boxed, obj, 5, 0)
        with pytest.raises(qn.ErrorInputParams, match="must not be negative"):
            qn.NonlinearCG(1e-8, x0).minimize(qn.ExactQuadratic(-1), obj, 5, 0)
        assert qn.ExactQuadratic().refresh_every() == 1
        chain.close()
    finally:
        obj.close()
        dense.close()
        lse.close()


def test_non_positive_curvature_leaves_x(qn):
    """a diagonal Q with one negative entry, started where the gradient points along it"""
    neg = SC.from_triplets(3, [0, 1, 2], [0, 1, 2], [1.0, -2.0, 1.0])
    obj = qn.SparseQuadratic(*neg, np.ones(3))
    x0 = np.array([0.0, 5.0, 0.0])
    try:
        for make in (lambda: qn.ProjectedGradientDescent(1e-10, x0, *LC.free_box(3)), lambda: qn.NonlinearCG(1e-10, x0), lambda: qn.LBFGS(1e-10, x0)):
            s = make()
            with pytest.raises(qn.AbnormalTermination, match="ExactQuadratic: non-positive curvature along the direction"):
                s.minimize(qn.ExactQuadratic(1), obj, 5, 0)
            assert np.array_equal(s.x(), x0)
            assert s.exact_state()["last_curvature"] < 0.0 and s.stats()["iterations"] == 0
    finally:
        obj.close()


def test_projected_lbfgs_meets_a_direction_that_does_not_descend(qn):
    """exact_cases.NOT_DESCENT_CASE: the three summation orders of the restatement agree on all its iterations and on its end"""
    method, name, n, r = EC.NOT_DESCENT_CASE
    ref, _, _, rstatus = EC.ref_case(EC.NOT_DESCENT_CASE)
    assert rstatus == "not_descent"
    obj = _objective(qn, name, n)
    try:
        s = _solver(qn, method, name, n, obj)
        s.set_trace(EC.WINDOW, with_x=True)
        with pytest.raises(qn.AbnormalTermination, match="ExactQuadratic: not a descent direction"):
            s.minimize(qn.ExactQuadratic(r), obj, EC.WINDOW, 0)
        tr, xs = s.trace()
        assert len(tr) == len(ref.trace)
        assert np.linalg.norm(s.x() - ref.x) <= 1e-9 * max(1.0, np.linalg.norm(ref.x))  # x stays at x_k
        assert np.array_equal(s.x(), xs[-1])
    finally:
        obj.close()


# ---- 7. warm restarts, 8. determinism ----
@pytest.mark.parametrize("method", ["cg-pr+", "lbfgs", "spg"])
@pytest.mark.parametrize("r", EC.REFRESH)
def test_two_calls_are_one(qn, method, r):
    name, n, k = "arrow", 2050, 5
    obj = _objective(qn, name, n)
    try:
        one = _solver(qn, method, name, n, obj)
        assert _run(qn, one, obj, r, 2 * k, trace=False) == "max_iter"
        two = _solver(qn, method, name, n, obj)
        assert _run(qn, two, obj, r, k, trace=False) == "max_iter"
        first = two.exact_state()["refreshes"]
        assert _run(qn, two, obj, r, k, trace=False) == "max_iter"
        assert one.x().tobytes() == two.x().tobytes()
        assert one.exact_state()["last_t"] == two.exact_state()["last_t"]
        assert one.exact_state()["refreshes"] == first + two.exact_state()["refreshes"]  # the count of accepted points since a true evaluation survives the call
    finally:
        obj.close()


@pytest.mark.parametrize("name", ["arrow", "dense"])
def test_determinism(qn, name):
    n = 2050
    one, two = _objective(qn, name, n), _objective(qn, name, n)
    try:
        out = []
        for obj in (one, one, two):
            s = _solver(qn, "cg-hz", name, n, obj)
            assert _run(qn, s, obj, 3, 20) == "max_iter"
            tr, xs = s.trace()
            out.append((xs.tobytes(), [x["t"] for x in tr], [x["f"] for x in tr]))
        assert out[0] == out[1] == out[2]
    finally:
        one.close()
        two.close()


# ---- 9. the C++ example ----
def test_cpp_example(qn):
    exe = os.path.join(ROOT, "examples", "exact_cg_example.bin")
    assert os.path.exists(exe), "build() compiles examples/exact_cg_example.cpp"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "exact cg example ok" in out.stdout, out.stdout + out.stderr
    fields = out.stdout.split("iterations:")[1].split()
    it, passes, refreshes = int(fields[0]), int(fields[2]), int(fields[4])
    counts = [EC.laplacian_cg(order)[0] for order in EC.ORDERS]
    margin = max(counts) - min(counts) + 2
    assert min(counts) - margin <= it <= max(counts) + margin and passes == it and refreshes >= 1
