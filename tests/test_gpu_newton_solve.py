"""GPU tests of Newton's dense solve on its own (csrc/qn_newton.hip.h, qn_lu.hip.h, qn_lu_split.hip.h, the drivers in qn_host_newton.hip.h):
one Newton iteration from x0 = 0 under NoSearch returns x_1 = 0 + 1 * d exactly, so the first row of the x-trace IS the kernel chain's
-(H^-1 g), bit for bit, for any H and g.  Each direction is held to the normwise backward error

    eta(H, x, g) = ||H x + g||_inf / (||H||_inf ||x||_inf + ||g||_inf) <= B(n) = max(n, 64) 2^-53,

residual in np.longdouble (newton_solve_cases.py: the families, the sizes at every block threshold, the bound; test_ref_newton_solve.py: LAPACK
sits under B(n) / 8 on all of them).  Families: A SPD through Cholesky (kappa up to 1e10), B the same through the pivoted LU, C dense Gaussian
(a swap in nearly every column), D scaled permutations (exact), E Cholesky failing late (then LU), F two factorisations in one solver, G one ulp
of asymmetry, H uniform scaling by 2^+-200, I n <= 5, J the second solve behind decrement_squared().

Largest eta / B(n) measured on one MI355X, per family (every test prints its own): A 0.017, B 0.005, C 0.018, E 0.028, F 0.010, G 0.002, H 0.006,
I 0.010; D exact; J at most 1.6e-4 of its bound (DESIGN.md 8.2 has LAPACK's next to them)."""
import numpy as np
import pytest

import newton_solve_cases as C

pytestmark = pytest.mark.gpu

_steps = {}


def newton_step(qn, H, g, *, via="host", options=()):
    """one Newton iteration from x0 = 0 with the step 1: (x_1 = -(H^-1 g) as the kernels left it, decrement_squared(), stats())"""
    n = len(g)
    s = qn.Newton(0.0, np.zeros(n))
    for name, value in options:
        s.set_option(name, value)
    s.set_trace(1, with_x=True)
    if via == "host":
        oracle = lambda x: qn.FuncEvalMultivariate(0.0, g).with_hessian(H)  # noqa: E731
    else:
        assert via == "quadratic"
        oracle = qn.Quadratic(H, -g)  # gradient H x - (-g) = g at x = 0; the matrix with the leading dimension n_pad
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.NoSearch(), oracle, 1, 20)
    tr, xs = s.trace()
    assert len(tr) == 1 and tr[0]["t"] == 1.0
    out = (xs[0].copy(), s.decrement_squared(), s.stats())
    s.close()
    return out


def step_of(qn, case):
    """the GPU's answer on one case, computed once (family J reads the same run's decrement)"""
    if case not in _steps:
        key, r, via, options = case
        _steps[case] = newton_step(qn, C.matrix(key), C.rhs(key, r), via=via, options=options)
    return _steps[case]


def _check_eta(case, x):
    H, g = C.matrix(case[0]), C.rhs(case[0], case[1])
    n = len(g)
    assert np.all(np.isfinite(x)), C.case_id(case)
    e = C.eta(H, x, g)
    print(f"eta {C.case_id(case)}: n={n} eta={e:.3e} B(n)={C.bound(n):.3e} ratio={e / C.bound(n):.4f}")
    assert e <= C.bound(n), (C.case_id(case), e, C.bound(n))
    return e


@pytest.mark.parametrize("case", C.A_CASES + C.A_QUAD_CASES, ids=C.case_id)
def test_a_spd_cholesky(qn, case):
    x, dec, _ = step_of(qn, case)
    _check_eta(case, x)
    assert dec is not None and dec > 0.0  # the Cholesky path (or the LU behind it) delivered a direction, not -g


@pytest.mark.parametrize("case", C.B_CASES, ids=C.case_id)
def test_b_spd_through_the_pivoted_lu(qn, case):
    x, dec, st = step_of(qn, case)
    _check_eta(case, x)
    assert dec is not None and st["newton_lu_sync_timeouts"] == 0
    chol = step_of(qn, (case[0], case[1], "host", ()))
    assert st["launches"] != chol[2]["launches"]  # another kernel chain than the Cholesky one ran


@pytest.mark.parametrize("case", C.C_CASES, ids=C.case_id)
def test_c_dense_gaussian_lu(qn, case):
    x, dec, st = step_of(qn, case)
    _check_eta(case, x)
    assert dec is not None and st["newton_lu_sync_timeouts"] == 0
    if case[3] == C.SPLIT:  # the split pivot chain: the same pivots and arithmetic as one workgroup's (tests/test_gpu_newton.py pins the variants to each other)
        assert np.array_equal(x, step_of(qn, (case[0], case[1], "host", ()))[0])


@pytest.mark.parametrize("case", C.D_CASES, ids=C.case_id)
def test_d_scaled_permutations_are_exact(qn, case):
    """every multiplier is zero and every pivot a power of two: perm, the right-hand side's permutation and the identity padding (never a
    pivot row) decide the answer, and it is exact"""
    key = case[0]
    x, dec, st = step_of(qn, case)
    x_exact = C.perm_exact(key[1], key[2])
    assert np.array_equal(x, x_exact), (C.case_id(case), int(np.sum(x != x_exact)))
    assert st["newton_lu_sync_timeouts"] == 0
    # z = H^-1 d is exact too (powers of two again); the dot product rounds
    _, p, d = C.scaled_permutation(key[1], key[2])
    z = np.empty(key[1], dtype=C.LD)
    z[p] = x_exact.astype(C.LD) / d.astype(C.LD)
    dec_exact = float(z @ x_exact.astype(C.LD))
    assert dec is not None
    assert abs(dec - dec_exact) <= key[1] * C.U * float(np.abs(z) @ np.abs(x_exact).astype(C.LD))


@pytest.mark.parametrize("case", C.E_CASES, ids=C.case_id)
def test_e_late_cholesky_failure_falls_through_to_lu(qn, case):
    """the first non-positive pivot at column c: 63 is the last column of the stand-alone chol_diag_inv_kernel, 64 the first of the copy inside
    chol_syrk_kernel (invL_next), 255 | 256 straddle an outer block, n = 900 fails with the look-ahead stream live"""
    key, r = case[0], case[1]
    H, g = C.matrix(key), C.rhs(key, r)
    x, dec, st = step_of(qn, case)
    _check_eta(case, x)
    assert dec is not None and st["newton_lu_sync_timeouts"] == 0
    d_newton = -np.linalg.solve(H, g)
    cosang = x @ d_newton / (np.linalg.norm(x) * np.linalg.norm(d_newton))
    assert cosang > 1.0 - 1e-9
    assert abs(x @ g) < (1.0 - 1e-6) * np.linalg.norm(x) * np.linalg.norm(g)  # not the gradient direction
    # and the same bits as the LU run alone: nothing of the abandoned Cholesky attempt is left in the factor
    lu = step_of(qn, (key, r, "host", C.LU))
    assert np.array_equal(x, lu[0]) and dec == lu[1]


@pytest.mark.parametrize("order", (0, 1), ids=("late-then-spd", "spd-then-late"))
def test_f_state_between_factorisations_in_one_solver(qn, order):
    """two iterations of one solver: a Cholesky that fails at column 256 and falls through to the LU, then an SPD matrix (and the reverse) --
    what the first leaves in newton_w's other triangle, newton_invl, newton_inv2 and newton_fail must not reach the second"""
    (k1, r1), (k2, r2) = C.F_ORDERS[order]
    H1, g1, H2, g2 = C.matrix(k1), C.rhs(k1, r1), C.matrix(k2), C.rhs(k2, r2)
    n = len(g1)

    def oracle(x):
        first = not np.any(x)
        return qn.FuncEvalMultivariate(0.0, g1 if first else g2).with_hessian(H1 if first else H2)

    s = qn.Newton(0.0, np.zeros(n))
    s.set_trace(2, with_x=True)
    with pytest.raises(qn.MaxIterReached):
        s.minimize(qn.NoSearch(), oracle, 2, 20)
    tr, xs = s.trace()
    assert len(tr) == 2 and s.k() == 2 and [r["t"] for r in tr] == [1.0, 1.0]
    s.close()
    _check_eta((k1, r1, "host", ()), xs[0])
    d2 = xs[1].astype(C.LD) - xs[0].astype(C.LD)
    assert np.all(np.isfinite(xs))
    e = C.eta(H2, d2, g2)
    print(f"eta second step of {C.case_id((k1, r1, 'host', ()))} -> {C.case_id((k2, r2, 'host', ()))}: eta={e:.3e} ratio={e / C.bound(n):.4f}")
    assert e <= C.bound(n), (e, C.bound(n))
    # the fresh solver's answer on the second system, for the record of what "no leftovers" means: the same step to the rounding of x_1 + d_2
    fresh = step_of(qn, (k2, r2, "host", ()))[0]
    assert np.max(np.abs(d2.astype(np.float64) - fresh)) <= 2.0 * C.U * np.max(np.abs(xs[1]))


def test_g_one_ulp_of_asymmetry_routes_to_lu(qn):
    x, dec, st = step_of(qn, C.G_CASE)
    _check_eta(C.G_CASE, x)
    chol = step_of(qn, C.G_SYMMETRIC)
    lu = step_of(qn, (C.G_SYMMETRIC[0], C.G_SYMMETRIC[1], "host", C.LU))
    # the launches of the forced LU run on the symmetric matrix, not the Cholesky run's
    assert st["launches"] == lu[2]["launches"] != chol[2]["launches"]
    assert st["host_syncs"] == lu[2]["host_syncs"]
    assert dec is not None


@pytest.mark.parametrize("case", C.H_CASES, ids=C.case_id)
def test_h_uniform_scaling(qn, case):
    """H and g times 2^200 and 2^-200: the measure is scale-free, and so is every step of the factorisations (no underflow, no overflow: the
    entries stay within 2^+-230)"""
    x, dec, _ = step_of(qn, case)
    _check_eta(case, x)
    base = step_of(qn, (case[0][1], case[1], "host", ()))
    assert np.array_equal(x, base[0])  # powers of two commute with every rounding of the chain
    assert dec == np.ldexp(base[1], -case[0][2])  # z = H^-1 d carries 2^-e


@pytest.mark.parametrize("case", C.I_CASES, ids=C.case_id)
def test_i_small_n_with_swaps(qn, case):
    x, dec, _ = step_of(qn, case)
    _check_eta(case, x)
    assert dec is not None


@pytest.mark.parametrize("case", C.J_CASES, ids=C.case_id)
def test_j_second_solve_behind_the_decrement(qn, case):
    """decrement_squared() = (H^-1 d) . d with d the GPU's own direction: the only check on the second solve's right-hand-side path
    (lu_vec_perm_kernel with sign = +1, the second newton_tri_solve).  Where kappa_inf(H) B(n) < 1e-3, a solve with backward error B(n) is
    within 2 kappa B / (1 - kappa B) of z* = H^-1 d (Higham Thm 7.2), and the dot product adds n 2^-53."""
    assert C.HAVE_LONGDOUBLE
    key = case[0]
    n = C.size(case)
    kb = C.kappa_inf(key) * C.bound(n)
    assert kb < C.J_LIMIT
    d, dec, _ = step_of(qn, case)
    z = C.solve_extended(key, d)
    dec_star = float(z @ d.astype(C.LD))
    tol = C.decrement_bound(n, float(np.max(np.abs(d))), float(np.max(np.abs(z))), kb)
    print(f"decrement {C.case_id(case)}: dec={dec:.17e} dec*={dec_star:.17e} |diff|={abs(dec - dec_star):.3e} bound={tol:.3e}")
    assert dec is not None and abs(dec - dec_star) <= tol, (C.case_id(case), dec, dec_star, tol)
