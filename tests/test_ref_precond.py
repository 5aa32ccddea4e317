"""CPU tests of the Hessian diagonal's restatement and bound (tests/ref_newton_pcg.py) and of the Jacobi-preconditioned NewtonCG restatement on the
badly scaled problems of tests/precond_cases.py: the checker accepts a correct float64 diagonal in three summation orders and rejects the planted
faults; every window the GPU tests use is licensed; the preconditioned runs converge and need at most half the plain runs' inner steps; the
counter-example (m < n, small mu) is recorded as one.

SEED_BASE = 7 (precond_cases): the only base tried; every window came out at 10 or more, or the whole run, so no other was needed.
RECORDED (this file prints them): inner totals plain / Jacobi -- dense (96, 64) 1302 / 406, dense (257, 200) 1942 / 472, sparse (96, 64) 794 / 182,
sparse (257, 200) 2964 / 362; the counter-example (40, 65): dense 213 / 276, sparse 173 / 227."""
import numpy as np
import pytest

import cg_cases as C
import logistic_cases as LC
import lse_hess_vec_cases as HV
import newton_cg_cases as NC
import precond_cases as PC
import ref_logistic as RL
import ref_newton_pcg as RP
import sparse_logistic_cases as SL

DENSE = [(1, 1), (3, 5), (40, 65), (257, 200), (7, 1030)]
ORDERS = ("numpy", "fsum", "reversed")


def _dot(order):
    return None if order == "numpy" else C.DOTS[order]


# ---- 1. the diagonal: a correct float64 value is inside the bound in any summation order ----
@pytest.mark.parametrize("m,n", DENSE)
def test_logistic_diagonal_inside_its_bound(m, n):
    for kind in ("edges", "unit"):
        pr, x, truth = LC.truth_at(m, n, 1.0, kind)
        a, y, w, mu = pr[:4]
        ms, bound = RP.logistic_diag_truth(a, y, w, mu, x, truth)
        for order in ORDERS:
            r = RP.ratio(RP.logistic_diag_at(a, y, w, mu, _dot(order))(x), ms, bound)
            print(f"logistic diagonal {(m, n)} {kind} {order}: max |M - M*| / bound = {r:.3f}")
            assert r <= 1.0, (kind, order, r)


@pytest.mark.parametrize("m,n", DENSE)
def test_lse_diagonal_inside_its_bound(m, n):
    a, c, mu, x0, _ = HV.problem(m, n)
    for scale in HV.SCALES:
        ms, bound = RP.lse_diag_truth(a, c, mu, scale * x0)
        for order in ORDERS:
            r = RP.ratio(RP.lse_diag_at(a, c, mu, _dot(order))(scale * x0), ms, bound)
            assert r <= 1.0, (scale, order, r)


def test_lse_diagonal_with_a_masked_row():
    m, n = HV.MASK_SHAPE
    for row in HV.MASK_ROWS.values():
        a, c, mu, x0, _ = HV.problem(m, n, row)
        ms, bound = RP.lse_diag_truth(a, c, mu, x0)
        assert RP.ratio(RP.lse_diag_at(a, c, mu)(x0), ms, bound) <= 1.0
        keep = np.arange(m) != row  # the value is that of the problem with the row deleted
        ms2, _ = RP.lse_diag_truth(a[keep], c[keep], mu, x0)
        assert RP.ratio(ms.astype(np.float64), ms2, bound) <= 1.0


@pytest.mark.parametrize("m,n", [(3, 5), (40, 65), (96, 64), (2050, 7)])
def test_sparse_diagonal_inside_its_bound(m, n):
    """the densified matrix: an absent entry adds an exact zero.  (40, 65): the last column is empty and M_j = mu exactly"""
    for kind in ("weighted", "edges"):
        pr, x, truth = SL.truth_at(m, n, 1.0, kind)
        ms, bound = RP.logistic_diag_truth(pr["a"], pr["y"], pr["w"], pr["mu"], x, truth)
        got = RP.logistic_diag_at(pr["a"], pr["y"], pr["w"], pr["mu"])(x)
        assert RP.ratio(got, ms, bound) <= 1.0
        if (m, n) == (40, 65):
            assert got[-1] == pr["mu"] and float(ms[-1]) == pr["mu"]


# ---- 2. the planted faults ----
def test_the_bound_rejects_planted_faults():
    m, n = 257, 200
    pr, x, truth = LC.truth_at(m, n, 1.0, "edges")
    a, y, w, mu = pr[:4]
    ms, bound = RP.logistic_diag_truth(a, y, w, mu, x, truth)
    d = RL.weights_f64(a, y, w, x)
    good = (a * a).T @ d + mu
    assert RP.ratio(good, ms, bound) <= 1.0
    assert RP.ratio(a.T @ d + mu, ms, bound) > 1e6           # a instead of a^2
    assert RP.ratio((a * a).T @ d, ms, bound) > 1e6           # mu dropped
    masked = np.nonzero(w == 0.0)[0]
    assert masked.size >= 2
    d_unit = RL.weights_f64(a, y, np.ones(m), x)
    counted = good + a[masked[0]] ** 2 * d_unit[masked[0]]    # one masked row counted
    assert RP.ratio(counted, ms, bound) > 1e6
    al, c, mul, x0, _ = HV.problem(m, n)
    ms, bound = RP.lse_diag_truth(al, c, mul, x0)
    z = al @ x0 + c
    p = np.exp(z - z.max())
    p /= p.sum()
    assert RP.ratio(RP.lse_diag_at(al, c, mul)(x0), ms, bound) <= 1.0
    assert RP.ratio((al * al).T @ p + mul, ms, bound) > 1e6   # - gbar^2 dropped


def test_minv_of_floors_what_is_not_positive_and_finite():
    minv, floored = RP.minv_of(np.array([4.0, 0.0, -2.0, np.inf, np.nan, 0.5]))
    assert floored == 4 and np.array_equal(minv, np.array([0.25, 1.0, 1.0, 1.0, 1.0, 2.0]))


@pytest.mark.parametrize("kind,m,n", [("dense", 96, 64), ("sparse", 257, 200)])
def test_the_window_rejects_minv_applied_twice(kind, m, n):
    ref = PC.ref_case(kind, m, n, "bt")[0]
    bad = PC.run_ref(kind, m, n, "bt", twice=True)[0]
    agree = NC.agreeing(ref, [bad], PC.GPU_TOL)[0]
    assert agree < min(PC.MIN_WINDOW, PC.window(kind, m, n, "bt")), agree


# ---- 3. the windows ----
@pytest.mark.parametrize("kind,m,n,ls", PC.CASES)
def test_every_window_is_licensed(kind, m, n, ls):
    w, worst, length = PC.licence(kind, m, n, ls)
    print(f"precond {kind} {(m, n)} {ls}: window {w} of {length}, worst disagreement between the orders {worst:.2e}")
    assert w >= min(PC.MIN_WINDOW, length), (w, length)
    assert worst <= PC.LICENCE


# ---- 4. convergence, and the half condition ----
@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("m,n", PC.SHAPES)
def test_jacobi_converges_in_at_most_half_the_inner_steps(kind, m, n):
    plain, _, st0 = PC.ref_case(kind, m, n, "bt", "none")
    pcg, _, st1 = PC.ref_case(kind, m, n, "bt", "jacobi")
    print(f"precond {kind} {(m, n)}: plain {len(plain.inner)} outer / {sum(plain.inner)} inner / {plain.why.count('cap')} capped; "
          f"Jacobi {len(pcg.inner)} / {sum(pcg.inner)} / {pcg.why.count('cap')}")
    assert st0 == "ok" and st1 == "ok"
    assert PC.final_gnorm(kind, m, n, pcg) < PC.TOL
    assert sum(pcg.inner) <= PC.HALF * sum(plain.inner), (sum(pcg.inner), sum(plain.inner))
    assert pcg.diag_passes == len(pcg.inner) and not any(pcg.floored)


@pytest.mark.parametrize("kind", PC.KINDS)
def test_the_counter_example_is_not_better(kind):
    """m < n with a small mu: the recorded expectation that Jacobi does NOT save inner steps there (both runs converge)"""
    m, n = PC.COUNTER
    plain, _, st0 = PC.ref_case(kind, m, n, "bt", "none")
    pcg, _, st1 = PC.ref_case(kind, m, n, "bt", "jacobi")
    print(f"precond counter-example {kind} {(m, n)}: plain {sum(plain.inner)} inner, Jacobi {sum(pcg.inner)}")
    assert st0 == "ok" and st1 == "ok" and PC.final_gnorm(kind, m, n, pcg) < PC.TOL
    assert sum(pcg.inner) >= sum(plain.inner)
