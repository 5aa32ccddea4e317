"""GPU tests of the sparse quadratic objective (qn.SparseQuadratic; kernels csrc/qn_sparse.hip.h): its evaluation against extended precision
with derived bounds, its determinism, and the O(n) solvers on it -- LBFGS / ProjectedLBFGS, SPG, projected gradient with GLLQuadratic,
BackTracking, BackTrackingB and StrongWolfe -- against the restatements on the host function of tests/sparse_cases.py.  Windows and the
tolerance (1e-9 max(1, ||x||), the family's) are licensed case by case by tests/test_ref_sparse.py.

THE EVALUATION'S BOUNDS are derived, not measured, and hold for any summation order with or without FMA.  With u = 2^-53, L_i the length of row i
and gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and 3.4): q_i is a sum of L_i products, g_i = q_i - b_i
one more operation, so |g_i - g_i*| <= gamma_(L_i + 1) (sum_j |Q_ij x_j| + |b_i|); f = sum_i x_i (1/2 q_i - b_i) adds n terms, each carrying its
row's L_i + 1 roundings and three more (the halving is exact, the subtraction, the product, and slack for a two-stage sum's extra level), so
|f - f*| <= gamma_(n + Lmax + 4) sum_i |x_i| (1/2 sum_j |Q_ij x_j| + |b_i|).  The reference is np.longdouble (u = 2^-64) -- its own error, the same
expressions with 2^-64 for u, is added to the bound -- and mpmath at n <= 7."""
import functools

import numpy as np
import pytest

import lbfgs_cases as LC
import ref_spg as R
import sparse_cases as SC

pytestmark = pytest.mark.gpu
PATH_VECTOR, PATH_PNEWTON, PATH_LBFGS = 64, 128, 1024
U = 2.0 ** -53
LANES = (0, 1, 2, 4, 8, 16, 32, 64)


def _gamma(k, u=U):
    return k * u / (1.0 - k * u)


# ---- 1. evaluation against extended precision ----
def _small_7():
    """n = 7: row 0 full, row 3 empty, the others a diagonal and one more entry; not symmetric (multiplied as given)"""
    rows = [0] * 7 + [1, 1, 2, 2, 4, 4, 5, 5, 6, 6]
    cols = list(range(7)) + [1, 4, 0, 2, 4, 6, 3, 5, 2, 6]
    vals = [1.5, -0.25, 0.125, 3.0, -2.0, 0.75, 1e-3] + [2.0, -1.0, 0.5, 4.0, 1.25, -3.0, 0.3, 2.5, -0.7, 5.0]
    return SC.from_triplets(7, rows, cols, vals)


EVAL_CASES = {
    "n1": lambda: (np.array([0, 1]), np.array([0]), np.array([2.5])),
    "n7_empty_and_full_row": _small_7,
    "tri2050": lambda: SC.tri(2050),
    "arrow2050": lambda: SC.arrow(2050),
    "band2050_20": lambda: SC.band(2050, 20),
    "band2050_350": lambda: SC.band(2050, 350),
    "arrow4100": lambda: SC.arrow(4100),
    "tri_2p21_plus_2": lambda: SC.tri(SC.BIG_N),
    "nnz0": lambda: (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)),
}


@functools.lru_cache(maxsize=None)
def _eval_reference(name):
    """(csr, b, x, g*, f*, bound on g per row, bound on f), the starred values in float64 nearest to the extended-precision ones"""
    indptr, cols, vals = (np.asarray(a) for a in EVAL_CASES[name]())
    indptr, cols = indptr.astype(np.int64), cols.astype(np.int64)
    n = indptr.size - 1
    rng = np.random.default_rng(17)
    x, b = rng.standard_normal(n), SC.rhs(n)
    lens = np.diff(indptr)
    rows = SC.row_index(indptr)
    absq = np.bincount(rows, weights=np.abs(vals * x[cols]), minlength=n)
    if n <= 7:
        import mpmath
        mpmath.mp.prec = 200
        q = [mpmath.mpf(0)] * n
        for r, c, v in zip(rows, cols, vals):
            q[r] += mpmath.mpf(float(v)) * mpmath.mpf(float(x[c]))
        g_ref = np.array([float(q[i] - mpmath.mpf(float(b[i]))) for i in range(n)])
        f_ref = float(sum(mpmath.mpf(float(x[i])) * (q[i] / 2 - mpmath.mpf(float(b[i]))) for i in range(n)))
        u_ref = 0.0
    else:
        prod = vals.astype(np.longdouble) * x[cols].astype(np.longdouble)
        q = np.zeros(n, dtype=np.longdouble)
        nonempty = lens > 0
        q[nonempty] = np.add.reduceat(prod, indptr[:-1][nonempty])  # (consecutive non-empty rows' starts delimit each row's entries)
        g_ld = q - b.astype(np.longdouble)
        f_ref = float(np.sum(x.astype(np.longdouble) * (q / 2 - b.astype(np.longdouble))))
        g_ref = g_ld.astype(np.float64)
        u_ref = 2.0 ** -64
    lmax = int(lens.max()) if lens.size else 0
    g_scale = absq + np.abs(b)
    f_scale = float(np.sum(np.abs(x) * (0.5 * absq + np.abs(b))))
    # + u per value: g* and f* above are the extended-precision values rounded to float64
    g_gamma = np.array([_gamma(int(k) + 1) + (_gamma(int(k) + 1, u_ref) if u_ref else 0.0) for k in lens])
    g_bound = g_gamma * g_scale + U * np.abs(g_ref)
    f_bound = (_gamma(n + lmax + 4) + (_gamma(n + lmax + 4, u_ref) if u_ref else 0.0)) * f_scale + U * abs(f_ref)
    return (indptr, cols, vals), b, x, g_ref, f_ref, g_bound, f_bound


@pytest.mark.parametrize("index_type", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("name", list(EVAL_CASES))
def test_evaluation_against_extended_precision(qn, name, index_type):
    (indptr, cols, vals), b, x, g_ref, f_ref, g_bound, f_bound = _eval_reference(name)
    obj = qn.SparseQuadratic(indptr.astype(index_type), cols.astype(index_type), vals, b)
    try:
        assert obj.nnz == vals.size and obj.n == b.size
        if name == "arrow4100":
            assert obj.n_long_rows >= 1
        if name in ("tri2050", "tri_2p21_plus_2", "n7_empty_and_full_row", "nnz0"):
            assert obj.n_long_rows == 0
        assert obj.symmetric == (0 if name == "n7_empty_and_full_row" else 1)
        auto = obj.lanes_per_row
        assert auto in LANES[1:]
        worst_g = worst_f = 0.0
        for lanes in LANES:
            obj.set_lanes_per_row(lanes)
            assert obj.lanes_per_row == (lanes or auto)
            f, g = obj(x)
            err = np.abs(g - g_ref)
            worst_g = max(worst_g, float(np.max(err / np.where(g_bound > 0.0, g_bound, 1.0))))
            worst_f = max(worst_f, abs(f - f_ref) / f_bound if f_bound > 0.0 else abs(f - f_ref))
            assert np.all(err <= g_bound), (lanes, int(np.argmax(err - g_bound)), float(np.max(err - g_bound)))
            assert abs(f - f_ref) <= f_bound, (lanes, f, f_ref, f_bound)
            if name == "nnz0":
                assert np.array_equal(g, -b)
        print(f"evaluation {name} {np.dtype(index_type).name}: auto lanes={auto} long rows={obj.n_long_rows} worst |g - g*| / bound={worst_g:.3f} worst |f - f*| / bound={worst_f:.3f}")
    finally:
        obj.close()


# ---- 2. determinism ----
@pytest.mark.parametrize("name", ["arrow4100", "band2050_350", "tri_2p21_plus_2"])
def test_determinism(qn, name):
    (indptr, cols, vals), b, x, _, _, _, _ = _eval_reference(name)
    one, two = qn.SparseQuadratic(indptr, cols, vals, b), qn.SparseQuadratic(indptr.copy(), cols.copy(), vals.copy(), b.copy())
    try:
        for lanes in (0, 2, 64):
            one.set_lanes_per_row(lanes)
            two.set_lanes_per_row(lanes)
            (f1, g1), (f2, g2), (f3, g3) = one(x), one(x), two(x)
            assert np.float64(f1).tobytes() == np.float64(f2).tobytes() == np.float64(f3).tobytes()
            assert g1.tobytes() == g2.tobytes() == g3.tobytes()
    finally:
        one.close()
        two.close()


# ---- 3. parity windows ----
def _compare(s, ref, window):  # (tests/test_gpu_spg.py's)
    tr, xs = s.trace()
    assert len(tr) == len(ref.trace) == window, (len(tr), len(ref.trace))
    for k in range(window):
        r = ref.trace[k]
        assert tr[k]["n_evals"] == r["n_evals"] and tr[k]["ls_iters"] == r["ls_iters"], (k, tr[k], r)
        assert abs(tr[k]["t"] - r["t"]) <= 1e-9 * abs(r["t"]), (k, tr[k]["t"], r["t"])
        assert np.linalg.norm(xs[k] - ref.trace_x[k]) <= 1e-9 * max(1.0, np.linalg.norm(ref.trace_x[k])), k
        assert abs(tr[k]["gnorm"] - r["gnorm"]) <= 1e-7 * max(1.0, r["gnorm"]), k


def _compare_updates(s, ref, window, fn, x0, lbfgs=True):
    """tests/test_gpu_lbfgs.py's: `updated`, s_norm and f of the trace against the restatement.  The bound on f: the iterates are licensed to 1e-9
    max(1, ||x||), so f(x_k) may move by ||g(x_k)||_2 times that (first order); on top, the device sums f in another order than numpy -- at most
    2^21 + 2 terms, blocked sums: 1e-11 max(1, |f|)."""
    tr, _ = s.trace()
    if lbfgs:
        assert [r["updated"] for r in tr[:window]] == ref.updated[:window]
    for k in range(window):
        if lbfgs:
            assert abs(tr[k]["s_norm"] - ref.trace[k]["s_norm"]) <= 1e-9 * max(1.0, ref.trace[k]["s_norm"]), k
        xk = ref.trace_x[k - 1] if k else R.box_projection(np.asarray(x0, dtype=np.float64), ref.lb, ref.ub)
        fr = ref.trace[k]["f"]
        bound = 1e-9 * max(1.0, float(np.linalg.norm(xk))) * float(np.linalg.norm(fn(xk)[1])) + 1e-11 * max(1.0, abs(fr))
        assert abs(tr[k]["f"] - fr) <= bound, (k, tr[k]["f"], fr, bound)


def _objective(qn, name, n, index_type=np.int32):
    indptr, cols, vals = SC.matrix(name, n)
    return qn.SparseQuadratic(indptr.astype(index_type), cols.astype(index_type), vals, SC.rhs(n))


def _ls(qn, case):
    kind, n, box = case[1], case[4], case[5]
    if kind == "gll":
        return qn.GLLQuadratic(1e-4, 10)
    if kind == "bt":
        return qn.BackTracking(1e-4, 0.5)
    if kind == "btb":
        return qn.BackTrackingB(1e-4, 0.5, *SC.box_of(n, box))
    ls = qn.StrongWolfe(1e-4, 0.9)
    for key, value in (case[6] if len(case) > 6 else ()):
        assert key == "t_max"
        ls.with_t_max(value)
    return ls


def _gpu(qn, case, oracle, iters, memoize=None):
    solver, _, m, name, n, box = case[:6]
    x0 = SC.start(n)
    lb, ub = SC.box_of(n, box)
    if solver == "lbfgs":
        s = qn.ProjectedLBFGS(SC.TOL, x0, lb, ub, m=m, memoize=memoize)
    elif solver == "spg":
        s = qn.SpectralProjectedGradient(SC.TOL, x0, oracle, lb, ub, memoize=memoize)
    else:
        s = qn.ProjectedGradientDescent(SC.TOL, x0, lb, ub)
        s.memoize = memoize
    s.set_trace(max(iters, 1), with_x=True)
    status = "ok"
    try:
        s.minimize(_ls(qn, case), oracle, iters, SC.MAX_LS)
    except qn.MaxIterReached:
        status = "max_iter"
    return s, status


def _check_window(qn, case, memoize=None):
    ref, rls, _, _ = SC.ref_case(case)
    w = SC.window(case)
    name, n = case[3], case[4]
    obj = _objective(qn, name, n)
    try:
        s, status = _gpu(qn, case, obj, w, memoize=memoize)
        assert status == "max_iter"
        st = s.stats()
        assert st["path"] & PATH_VECTOR and not st["path"] & PATH_PNEWTON
        assert bool(st["path"] & PATH_LBFGS) == (case[0] == "lbfgs")
        assert st["obj_bytes"] == st["oracle_evals"] * (12 * obj.nnz + 4 * (n + 1) + 24 * n)
        if w == 0:
            assert case in SC.WOLFE_KNIFE_EDGE  # nothing is licensed to compare (sparse_cases.py says why): the call itself, its path and its accounting
            return s, ref, w
        ref_w = type("W", (), dict(trace=ref.trace[:w], trace_x=ref.trace_x[:w]))
        _compare(s, ref_w, w)
        fn, x0 = SC.problem(name, n)
        _compare_updates(s, ref, w, fn, x0, lbfgs=case[0] == "lbfgs")
        if case[1] == "wolfe":
            tr, _ = s.trace()
            for k in range(w):
                assert tr[k]["ls_cases"] == rls.history[k]["ls_cases"], (k, oct(tr[k]["ls_cases"]), oct(rls.history[k]["ls_cases"]))
        return s, ref, w
    finally:
        obj.close()


@pytest.mark.parametrize("case", SC.FREE_CASES, ids=str)
def test_parity_window(qn, case):
    s, ref, w = _check_window(qn, case)
    if case[0] == "lbfgs" and w:
        assert s.memory == case[2] and s.stored_pairs() == min(case[2], sum(ref.updated[:w]))


@pytest.mark.parametrize("case", SC.BOX_CASES, ids=str)
def test_projected_parity_window(qn, case):
    s, ref, w = _check_window(qn, case)
    n, box = case[4], case[5]
    lb, ub = SC.box_of(n, box)
    x = s.x()
    assert np.all(x >= lb - SC.box_slack(box)) and np.all(x <= ub + SC.box_slack(box))  # (inside, but for the rounding of x + t d: sparse_cases.box_slack)
    assert 0 < int(np.sum((x == lb) | (x == ub))) < n


@pytest.mark.parametrize("case", [("lbfgs", "gll", 5, "tri", 2050, None), ("lbfgs", "bt", 5, "arrow", 2050, None), ("spg", "gll", 0, "arrow", 2050, None),
                                  ("pgd", "bt", 0, "tri", 7, None), ("lbfgs", "wolfe", 5, "arrow", 7, None)], ids=str)
def test_memoize_and_counts(qn, case):
    w = SC.window(case)
    ref_w, _, o_w, _ = SC.run_ref(case, iters=w)
    xs, evals = [], []
    for memo in (0, 1):
        s, _, _ = _check_window(qn, case, memoize=memo)
        xs.append(s.trace()[1].copy())
        st = s.stats()
        assert st["total_oracle_calls"] == o_w.calls  # the restatement's call sequence (SPG: its constructor's call included), whatever is memoised
        evals.append(st["total_oracle_evals"])
    assert xs[0].tobytes() == xs[1].tobytes()
    assert evals[0] == o_w.calls and evals[1] < evals[0]
    if case[0] == "lbfgs":  # memoised: the loop top's and the update's evaluations are the line search's last trial -- one evaluation per trial, one for x0
        assert evals[1] == 1 + sum(r["ls_iters"] for r in ref_w.trace[:w])


# ---- 4. dense and sparse say the same ----
def test_dense_and_sparse_agree(qn):
    case = ("lbfgs", "bt", 5, "tri", 2050, None)
    w = SC.window(case)
    csr = SC.tri(2050)
    sparse, dense = _objective(qn, "tri", 2050), qn.Quadratic(SC.dense(csr), SC.rhs(2050))
    try:
        (a, sa), (b, sb) = _gpu(qn, case, sparse, w), _gpu(qn, case, dense, w)
        assert sa == sb == "max_iter"
        (ta, xa), (tb, xb) = a.trace(), b.trace()
        assert len(ta) == len(tb) == w
        assert [r["updated"] for r in ta] == [r["updated"] for r in tb]
        for k in range(w):
            assert np.linalg.norm(xa[k] - xb[k]) <= 1e-9 * max(1.0, np.linalg.norm(xb[k])), k
    finally:
        sparse.close()
        dense.close()


# ---- 5. size ----
def test_parity_row_loop_wraps(qn):
    """tri(2^21 + 2): 2048 regular workgroups walk ~1024 rows each; LBFGS(m = 3) + BackTracking, 5 iterations"""
    ref, _, _, _ = SC.ref_big()
    n = SC.BIG_N
    case = ("lbfgs", "bt", SC.BIG_M, "tri", n, None)
    obj = _objective(qn, "tri", n)
    try:
        s, status = _gpu(qn, case, obj, SC.BIG_WINDOW)
        assert status == "max_iter"
        _compare(s, ref, SC.BIG_WINDOW)
        fn, x0 = SC.problem("tri", n)
        _compare_updates(s, ref, SC.BIG_WINDOW, fn, x0)
        assert s.stored_pairs() == SC.BIG_M
    finally:
        obj.close()


# ---- 6. errors ----
def _raw_create(qn, n, nnz, indptr, indices, index_bytes, data, b):
    import ctypes as C
    A = qn._abi
    h = C.c_void_p()

    def vp(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def dp(a):
        return None if a is None else a.ctypes.data_as(A.dp)
    ctx = qn.default_context()
    st = A.lib().qn_sparse_quadratic_create(ctx.h, n, nnz, vp(indptr), vp(indices), index_bytes, dp(data), dp(b), C.byref(h))
    if st == A.OK:
        A.lib().qn_objective_destroy(h)
    qn.solver._check(st)


def test_invalid_inputs(qn):
    ip, ci = np.array([0, 2, 3, 5], dtype=np.int64), np.array([0, 1, 1, 0, 2], dtype=np.int64)
    va, b = np.arange(1.0, 6.0), np.ones(3)
    _raw_create(qn, 3, 5, ip, ci, 8, va, b)  # the valid one
    for args in ((3, 5, None, ci, 8, va, b), (3, 5, ip, None, 8, va, b), (3, 5, ip, ci, 8, None, b), (3, 5, ip, ci, 8, va, None),
                 (0, 0, ip, ci, 8, va, b),                      # n == 0
                 (3, 5, ip, ci, 2, va, b), (3, 5, ip, ci, 0, va, b), (3, 5, ip, ci, 16, va, b),  # index_bytes
                 ((1 << 30) + 1, 5, ip, ci, 8, va, b),          # n > 2^30 (checked before anything is read)
                 (3, 1 << 31, ip, ci, 8, va, b)):               # nnz > 2^31 - 1
        with pytest.raises(qn.ErrorInputParams):
            _raw_create(qn, *args)
    bad = {
        "row_ptr[0] != 0": ([1, 2, 3, 5], ci),
        "row_ptr[n] != nnz": ([0, 2, 3, 4], ci),
        "row_ptr[n] > nnz": ([0, 2, 3, 6], ci),
        "decreasing row_ptr": ([0, 3, 2, 5], ci),
        "column == n": (ip, [0, 1, 1, 0, 3]),
        "negative column": (ip, [0, 1, 1, -1, 2]),
        "unsorted columns": (ip, [1, 0, 1, 0, 2]),
        "duplicate column": (ip, [0, 0, 1, 0, 2]),
    }
    for why, (p, c) in bad.items():
        for t in (np.int32, np.int64):
            with pytest.raises(qn.ErrorInputParams):
                qn.SparseQuadratic(np.array(p, dtype=t), np.array(c, dtype=t), va, b)
    with pytest.raises(qn.ErrorInputParams):
        qn.SparseQuadratic(ip[:-1], ci, va, b)  # indptr does not have n + 1 entries
    with pytest.raises(qn.ErrorInputParams):
        qn.SparseQuadratic(ip.astype(np.float64), ci, va, b)
    # other integer types are converted
    small = qn.SparseQuadratic(ip.astype(np.uint16), ci.astype(np.int16), va, b)
    assert small.nnz == 5
    for lanes in (3, -1, 128):
        with pytest.raises(qn.ErrorInputParams):
            small.set_lanes_per_row(lanes)
    small.close()


def test_non_symmetric_is_multiplied_as_given(qn):
    ip, ci = np.array([0, 2, 3, 5], dtype=np.int32), np.array([0, 1, 1, 0, 2], dtype=np.int32)
    va, b, x = np.arange(1.0, 6.0), np.array([0.5, -1.0, 2.0]), np.array([1.0, -2.0, 3.0])
    obj = qn.SparseQuadratic(ip, ci, va, b)
    assert obj.symmetric == 0 and obj.nnz == 5
    q = SC.dense((ip.astype(np.int64), ci.astype(np.int64), va))
    f, g = obj(x)
    assert np.array_equal(g, q @ x - b)  # (small integers: exact)
    assert f == 0.5 * float(x @ (q @ x)) - float(b @ x)
    sym = qn.SparseQuadratic(*SC.tri(7), SC.rhs(7))
    assert sym.symmetric == 1
    # the same pattern with one value off by an ulp is not symmetric bit for bit
    indptr, cols, vals = SC.tri(7)
    vals = vals.copy()
    vals[1] = np.nextafter(vals[1], 0.0)
    assert qn.SparseQuadratic(indptr, cols, vals, SC.rhs(7)).symmetric == 0


def test_unsupported_methods_and_calls(qn):
    n = 7
    obj = _objective(qn, "tri", n)
    x0 = SC.start(n)
    lb, ub = LC.free_box(n)
    bt = qn.BackTracking(1e-4, 0.5)
    for solver in (qn.BFGS(1e-8, x0), qn.GradientDescent(1e-8, x0), qn.Newton(1e-8, x0)):
        with pytest.raises(qn.ErrorInputParams):
            solver.minimize(bt, obj, 5, 20)
    with pytest.raises(qn.ErrorInputParams, match="Hessian not available"):
        qn.ProjectedNewton(1e-8, x0, lb, ub).minimize(bt, obj, 5, 20)
    with pytest.raises(qn.ErrorInputParams, match="More-Thuente"):
        qn.LBFGS(1e-8, x0).minimize(qn.MoreThuente(), obj, 5, 20)
    with pytest.raises(qn.ErrorInputParams, match="no dense rows"):
        obj.rows(0, 1)
    with pytest.raises(qn.ErrorInputParams, match="no dense rows"):
        obj.hessian(x0)
    with pytest.raises(qn.ErrorInputParams):
        obj(np.zeros(n + 1))
    # the info call and the lanes setter belong to this kind
    dense = qn.Quadratic(np.eye(2), np.ones(2))
    import ctypes as C
    with pytest.raises(qn.ErrorInputParams):
        qn.solver._check(qn._abi.lib().qn_objective_sparse_info(dense.h, None, None, None, None))
    with pytest.raises(qn.ErrorInputParams):
        qn.solver._check(qn._abi.lib().qn_sparse_quadratic_set_lanes_per_row(dense.h, 4))
    nnz = C.c_size_t()
    qn.solver._check(qn._abi.lib().qn_objective_sparse_info(obj.h, C.byref(nnz), None, None, None))  # NULL out-pointers are skipped
    assert nnz.value == 3 * n - 2
    obj.close()
    obj.close()
    with pytest.raises(qn.ErrorInputParams):
        obj(x0)
    with pytest.raises(qn.ErrorInputParams):
        obj.nnz
    with pytest.raises(qn.ErrorInputParams):
        obj.set_lanes_per_row(4)
    with pytest.raises(qn.ErrorInputParams):
        qn.LBFGS(1e-8, x0).minimize(bt, obj, 5, 20)


def test_from_scipy(qn):
    sp = pytest.importorskip("scipy.sparse")
    n = 2050
    indptr, cols, vals = SC.arrow(n)
    rows = SC.row_index(indptr)
    perm = np.random.default_rng(3).permutation(vals.size)  # a COO in scrambled order, one entry split in two: sorted and summed on the way in
    r, c, v = rows[perm], cols[perm], vals[perm].copy()
    v[0] *= 0.5
    coo = sp.coo_matrix((np.concatenate([v, v[:1]]), (np.concatenate([r, r[:1]]), np.concatenate([c, c[:1]]))), shape=(n, n))
    b, x = SC.rhs(n), SC.start(n)
    a, ref = qn.SparseQuadratic.from_scipy(coo, b), qn.SparseQuadratic(indptr, cols, vals, b)
    assert a.nnz == ref.nnz == vals.size and a.symmetric == 1
    (fa, ga), (fr, gr) = a(x), ref(x)
    assert fa == fr and ga.tobytes() == gr.tobytes()


def test_world_above_one_is_rejected(qn):
    from thread_ranks import run_ranks

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        with pytest.raises(qn.ErrorInputParams, match="one rank"):
            qn.SparseQuadratic(*SC.tri(32), SC.rhs(32), ctx=ctx)
        ctx.close()
        return True
    assert run_ranks(2, body, timeout=60.0) == [True, True]


# ---- 7. warm restart ----
@pytest.mark.parametrize("memoize", [0, 1])
def test_warm_restart(qn, memoize):
    n = 2050
    case = ("lbfgs", "gll", 5, "arrow", n, None)
    obj = _objective(qn, "arrow", n)
    x0 = SC.start(n)
    one, _ = _gpu(qn, case, obj, 10, memoize=memoize)
    two = qn.LBFGS(SC.TOL, x0, m=5, memoize=memoize)
    ls = qn.GLLQuadratic(1e-4, 10)
    evals = 0
    for _ in range(2):
        with pytest.raises(qn.MaxIterReached):
            two.minimize(ls, obj, 5, SC.MAX_LS)
        assert two.k() == 5
        evals += two.stats()["oracle_evals"]
    assert one.x().tobytes() == two.x().tobytes()
    assert two.stored_pairs() == one.stored_pairs() == 5 and two.gamma() == one.gamma()
    if memoize:
        assert evals == one.stats()["oracle_evals"]  # the second call starts from the memo of the first one's last evaluation
    spg_one = qn.SpectralProjectedGradient(SC.TOL, x0, obj, *LC.free_box(n))
    spg_two = qn.SpectralProjectedGradient(SC.TOL, x0, obj, *LC.free_box(n))
    with pytest.raises(qn.MaxIterReached):
        spg_one.minimize(qn.GLLQuadratic(1e-4, 10), obj, 10, SC.MAX_LS)
    gl = qn.GLLQuadratic(1e-4, 10)
    for _ in range(2):
        with pytest.raises(qn.MaxIterReached):
            spg_two.minimize(gl, obj, 5, SC.MAX_LS)
    assert spg_one.x().tobytes() == spg_two.x().tobytes()
    obj.close()
