"""CPU tests that license the cases of tests/test_gpu_newton_solve.py (newton_solve_cases.py): on every case LAPACK's own solve must sit a
factor of 8 inside the bound B(n) = max(n, 64) 2^-53 the GPU kernels are held to, so that a GPU failure is a finding about the kernels and
not about the case; the SPD matrices must pass a Cholesky factorisation, each late-failure matrix must fail one exactly at its column, the
scaled permutations must be solved exactly, and every block threshold of csrc/qn_host_newton.hip.h must be in the lists.

Largest eta / B(n) of LAPACK per family, as printed by test_lapack_sits_inside_the_bound (f64 `numpy.linalg.solve`, residual in np.longdouble):
A 0.015, B 0.005, C 0.015, E 0.020, G 0.001, H 0.006, I 0.009 (DESIGN.md 8.2 puts the MI355X's next to them)."""
import numpy as np
import pytest

import newton_solve_cases as C

FAMILIES = {"A": C.A_CASES + C.A_QUAD_CASES, "B": C.B_CASES, "C": C.C_CASES, "E": C.E_CASES, "G": [C.G_CASE], "H": C.H_CASES, "I": C.I_CASES}


def test_extended_precision_is_available():
    """the residuals need a 64-bit significand (x87 extended); without it the measure falls back to mpmath up to n = 257 and skips above"""
    assert np.finfo(np.longdouble).nmant >= 63


def test_the_measure_by_hand():
    h = np.array([[2.0, 0.0], [0.0, 4.0]])
    g = np.array([-2.0, -4.0])
    assert C.eta(h, np.array([1.0, 1.0]), g) == 0.0
    assert C.eta(h, np.array([1.0, 1.5]), g) == 2.0 / (4.0 * 1.5 + 4.0)
    # a residual below f64's resolution of its terms is still seen: (1 + 2^-30)^2 - (1 + 2^-29) = 2^-60
    a = 1.0 + 2.0 ** -30
    assert C.residual_inf(np.array([[a]]), np.array([a]), np.array([-(1.0 + 2.0 ** -29)])) == 2.0 ** -60
    assert C._residual_mp(np.array([[a]]), np.array([a]), np.array([-(1.0 + 2.0 ** -29)])) == 2.0 ** -60
    assert C.bound(6) == C.bound(64) == 64 * 2.0 ** -53 and C.bound(2049) == 2049 * 2.0 ** -53


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_lapack_sits_inside_the_bound(family):
    worst = 0.0
    for case in FAMILIES[family]:
        key, r, _, _ = case
        h, g = C.matrix(key), C.rhs(key, r)
        n = h.shape[0]
        x = -np.linalg.solve(h, g)
        e = C.eta(h, x, g)
        worst = max(worst, e / C.bound(n))
        assert np.all(np.isfinite(x)) and e <= C.bound(n) / 8.0, (C.case_id(case), e, C.bound(n) / 8.0)
    print(f"family {family}: largest eta / B(n) of LAPACK = {worst:.3f}")


def test_spd_matrices_pass_cholesky_and_are_symmetric_bit_for_bit():
    for key in sorted({c[0] for c in C.A_CASES + C.A_QUAD_CASES + C.B_CASES} | {C.F_SPD[0]}):
        h = C.matrix(key)
        assert np.array_equal(h, h.T)
        np.linalg.cholesky(h)
        ev = np.linalg.eigvalsh(h)
        assert 0.5 * key[2] <= ev[-1] / ev[0] <= 2.0 * key[2]  # the condition number asked for


def _first_bad_pivot(h):
    """unblocked (column by column, left-looking) Cholesky of the lower triangle: the column of the first non-positive pivot, or -1"""
    n = h.shape[0]
    l = np.zeros((n, n))
    for k in range(n):
        col = h[k:, k] - l[k:, :k] @ l[k, :k]
        if not col[0] > 0.0:
            return k
        l[k:, k] = col / np.sqrt(col[0])
    return -1


@pytest.mark.parametrize("n,c", C.E_PAIRS)
def test_late_failure_matrices_fail_cholesky_exactly_at_their_column(n, c):
    h = C.matrix(("late", n, c))
    assert np.array_equal(h, h.T) and _first_bad_pivot(h) == c
    good = h.copy()
    good[c, c] = 4.0
    assert _first_bad_pivot(good) == -1 and np.linalg.cond(good) < 1.5
    assert np.linalg.cond(h) < 10.0  # indefinite and well conditioned: the cosine test against LAPACK is a tolerance-level statement


def test_late_failures_are_late():
    cols = [c for _, c in C.E_PAIRS]
    assert min(cols) == 0 and sum(c > 0 for c in cols) == 9
    assert {(130, 63), (130, 64), (300, 255), (300, 256)} <= set(C.E_PAIRS)  # the last column of the stand-alone diagonal kernel, the first of the fused site, an outer block's edge
    assert any(n >= 769 and c >= 256 for n, c in C.E_PAIRS)  # with the look-ahead stream live


@pytest.mark.parametrize("n", C.D_SIZES)
@pytest.mark.parametrize("kind", C.PERMS)
def test_scaled_permutations_are_solved_exactly(n, kind):
    key = ("perm", n, kind)
    h, g = C.matrix(key), C.rhs(key, "ints")
    x_exact = C.perm_exact(n, kind)
    assert not np.array_equal(h, h.T)  # straight to the pivoted LU
    assert np.array_equal(-np.linalg.solve(h, g), x_exact)
    assert C.eta(h, x_exact, g) == 0.0
    _, p, d = C.scaled_permutation(n, kind)
    assert sorted(p) == list(range(n)) and np.all(np.abs(np.log2(np.abs(d))) <= 20) and np.all(np.log2(np.abs(d)) % 1 == 0)
    assert np.all((g >= 1) & (g < 2 ** 20) & (g == np.round(g)))
    if kind == "cyclic":  # column k's only entry is in row k + 1: the row that starts at 0 moves down one place per column
        assert all(h[k + 1, k] != 0.0 for k in range(n - 1)) and h[0, n - 1] != 0.0
    if kind == "reversal":
        assert all(h[n - 1 - k, k] != 0.0 for k in range(n))


def test_small_matrices_need_swaps():
    for n in C.I_SIZES:
        h = C.matrix(("small", n))
        assert h[0, 0] == 0.0  # elimination without a swap divides by zero at once
        assert all(np.argmax(np.abs(h[i])) != i for i in range(n))  # the dominant entry of every row is off the diagonal


def test_one_ulp_of_asymmetry():
    h, s = C.matrix(C.G_CASE[0]), C.matrix(C.G_SYMMETRIC[0])
    diff = np.argwhere(h != s)
    assert diff.tolist() == [[256, 0]] and h[256, 0] == np.nextafter(s[256, 0], np.inf)
    assert np.array_equal(C.rhs(C.G_CASE[0]), C.rhs(C.G_SYMMETRIC[0]))


def test_uniform_scaling_is_exact():
    for key, r, _, _ in C.H_CASES:
        base, e = key[1], key[2]
        assert np.array_equal(np.ldexp(C.matrix(key), -e), C.matrix(base)) and np.array_equal(np.ldexp(C.rhs(key, r), -e), C.rhs(base, r))
        assert np.all(np.isfinite(C.matrix(key))) and np.min(np.abs(C.matrix(key)[C.matrix(key) != 0.0])) > 2.0 ** -1000


def test_case_lists_hold_every_threshold():
    a = {C.size(c) for c in C.A_CASES}
    assert {6, 63, 64, 65, 257, 512, 513, 769, 1100} <= a
    assert {c[0][2] for c in C.A_CASES} == {1e2, 1e6, 1e10} and {c[1] for c in C.A_CASES} == {"normal", "range"}
    assert len(C.A_CASES) == 9 * 3 * 2
    assert {C.size(c) for c in C.A_QUAD_CASES} == {65, 777} and all(c[2] == "quadratic" for c in C.A_QUAD_CASES)
    assert {(C.size(c), c[0][2]) for c in C.B_CASES} == {(n, k) for n in (65, 513, 769) for k in (1e2, 1e10)}
    assert all(c[3] == C.LU for c in C.B_CASES)
    assert [C.size(c) for c in C.C_CASES if not c[3]] == [6, 65, 449, 513, 1025, 2049]
    assert [C.size(c) for c in C.C_CASES if c[3] == C.SPLIT] == [449, 1025]
    assert max(C.size(c) for c in C.ALL_CASES) == 2049
    assert {C.size(c) for c in C.D_CASES} == {70, 449, 1025} and len(C.D_CASES) == 9
    assert len(C.E_CASES) == 10 and {C.size(c) for c in C.I_CASES} == {2, 3, 4, 5}
    assert C.size(C.G_CASE) == 257 and {C.size(c) for c in C.H_CASES} == {257, 449} and {c[0][2] for c in C.H_CASES} == {200, -200}
    # the thresholds themselves, restated from csrc/qn_host_newton.hip.h (QN_NB = 64, QN_TS = 512, KB = 256, QN_LU_PT = 512 threads per panel)
    pad64 = lambda n: -(-n // 64) * 64  # noqa: E731
    assert pad64(512) == 512 and pad64(513) > 512  # newton_big
    assert -(-pad64(513) // 512) * 512 == 1024
    assert -(-pad64(257) // 256) == 2 and -(-1024 // 256) >= 4 and -(-pad64(512) // 256) < 4  # outer blocks; look-ahead from n = 513 (padded to 1024) and 769
    assert pad64(449) // 64 == 8 and pad64(448) // 64 == 7  # LU look-ahead
    # rows per thread of the first (tallest) panel, ceil(nlu / 512): the instantiations 1 | 2 | 4 | 8 change behind heights 512, 1024, 2048
    assert [-(-pad64(n) // 512) for n in (449, 512, 513, 1024, 1025, 2048, 2049)] == [1, 1, 2, 2, 3, 4, 5]
    ids = [C.case_id(c) for c in C.ALL_CASES]
    assert len(set(ids)) == len(ids)


def test_second_solve_cases_are_the_ones_inside_the_limit():
    inside = [c for c in C.J_CANDIDATES if C.kappa_inf(c[0]) * C.bound(C.size(c)) < C.J_LIMIT]
    assert inside == C.J_CASES and len(C.J_CASES) == len(C.J_CANDIDATES) - 10 - 4  # (kappa = 1e10 at n >= 257: 5 sizes x 2 right-hand sides of A, 2 x 2 of B)
    for c in C.J_CASES:  # where LAPACK's inverse is the preconditioner of solve_extended, its contraction kappa 2^-53 is far below 1
        assert C.kappa_inf(c[0]) * C.U < 1e-4


def test_second_solve_reference():
    """solve_extended (family J's z*): where kappa_inf B(n) < 1e-3 the refinement reaches the residual of an extended-precision solve and has converged"""
    for key in (("spd", 65, 1e2), ("spd", 65, 1e10), ("gauss", 65)):
        h = C.matrix(key)
        n = h.shape[0]
        if not C.kappa_inf(key) * C.bound(n) < C.J_LIMIT:
            continue
        d = C.rhs(key, "normal")
        z = C.solve_extended(key, d)
        r = np.max(np.abs(d.astype(C.LD) - h.astype(C.LD) @ z))
        assert float(r) <= 8 * n * float(np.finfo(C.LD).eps) * C.norm_inf(h) * float(np.max(np.abs(z)))
        # converged: one sweep fewer moves z by no more than the floor kappa_inf eps_longdouble -- five decimal orders inside the
        # 2 kappa_inf B(n) that family J allows, whatever kappa_inf is
        floor = 8 * C.kappa_inf(key) * float(np.finfo(C.LD).eps)
        assert float(np.max(np.abs(z - C.solve_extended(key, d, sweeps=5)))) <= floor * float(np.max(np.abs(z)))
        assert floor <= 1e-4 * 2 * C.kappa_inf(key) * C.bound(n)
    assert C.kappa_inf(("spd", 65, 1e2)) * C.bound(65) < C.J_LIMIT
    n, d, z, kb = 100, 2.0, 3.0, 1e-4
    assert C.decrement_bound(n, d, z, kb) == n * d * z * (2 * kb / (1 - kb) + n * 2.0 ** -53)
