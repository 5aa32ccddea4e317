"""CPU tests of tests/ref_multinomial.py and tests/multinomial_cases.py: the float64 restatement is inside the derived bounds of the longdouble truth
in three summation orders at every shape and scale, the checker rejects planted faults, and the NewtonCG / family windows the GPU tests use are
licensed for the restatement ALONE (newton_cg_cases' method and constants)."""
import math

import numpy as np
import pytest

import cg_cases as C
import multinomial_cases as MC
import ref_multinomial as RM

ORDERS = ("numpy", "fsum", "reversed")


def _restated(pr, x, order):
    a, y, w, k, mu, _, v = pr
    dot = None if order == "numpy" else C.DOTS[order]
    f, g = RM.multinomial_fn(a, y, w, k, mu, dot)(x)
    q = RM.multinomial_hess_vec_at(a, y, w, k, mu, dot)(x)(v)
    c = float(v @ q) if dot is None else float(dot(v, q))
    return dict(f=f, g=g, p=RM.probabilities_f64(a, y, w, k, x, dot), q=q, c=c)


@pytest.mark.parametrize("m,n,k", [s for s in MC.SHAPES if s[0] * s[1] * s[2] <= 64 * 41 * 17])
def test_the_restatement_is_inside_the_bounds_in_three_orders(m, n, k):
    for kind, scales in (("weighted", MC.SCALES), ("unit", [1.0]), ("edges", [1.0]), ("absent", [1.0])):
        for scale in scales:
            pr, x, truth = MC.truth_at(m, n, k, scale, kind)
            for order in ORDERS:
                r = RM.ratios(_restated(pr, x, order), truth)
                assert all(v <= 1.0 for v in r.values()), (kind, scale, order, r)


def test_the_wide_shapes_in_numpy_order():
    for (m, n, k) in [s for s in MC.SHAPES if s[0] * s[1] * s[2] > 64 * 41 * 17] + MC.CUT_SHAPES:
        pr, x, truth = MC.truth_at(m, n, k, 1.0)
        r = RM.ratios(_restated(pr, x, "numpy"), truth)
        assert all(v <= 1.0 for v in r.values()), ((m, n, k), r)


def test_saturation_and_a_masked_row_that_overflows():
    a, y, w, k, mu, x, spread = MC.saturated_problem()
    f, g = RM.multinomial_fn(a, y, w, k, mu)(x)
    p = RM.probabilities_f64(a, y, w, k, x)
    assert np.isfinite(f) and np.all(np.isfinite(g))
    assert p[0, 1] == 0.0 and p[0, 2] == 0.0 and p[0, 0] == 1.0 and np.all(p[2] == 0.0)
    mild = math.log(math.exp(0.5) + math.exp(-0.5) + math.exp(0.125)) + 0.5
    assert abs(f - (spread + mild + 0.5 * mu * float(x @ x))) <= 1e-9 * f
    pr = MC.variant(17, 7, 3, "overflow")
    xo = MC.overflow_point(pr)
    got = _restated(pr, xo, "numpy")
    assert np.isfinite(got["f"]) and np.all(np.isfinite(got["g"])) and np.all(np.isfinite(got["q"])) and np.all(got["p"][17 // 2] == 0.0)
    live = np.delete(np.arange(17), 17 // 2)  # the value is that of the problem with the row deleted
    f2, g2 = RM.multinomial_fn(pr[0][live], pr[1][live], pr[2][live], 3, pr[4])(xo)
    assert f2 == got["f"] and np.array_equal(g2, got["g"])


def _faulty(kind, pr, x):
    """the restatement with one planted fault"""
    a, y, w, k, mu, _, v = pr
    n = a.shape[1]
    good = _restated(pr, x, "numpy")
    if kind == "wrong label column":
        return _restated((a, (y + 1) % k, w, k, mu, None, v), x, "numpy")
    if kind == "p_y - 1 with a dropped class":
        z = a @ x.reshape(k, n).T
        e = np.exp(z - z.max(axis=1)[:, None])
        s = e.sum(axis=1)
        rows = np.arange(a.shape[0])
        drop = np.where(y == k - 1, k - 2, k - 1)  # the last class that is not the label never enters Sn
        c = w[:, None] * e / s[:, None]
        c[rows, y] = -(w * ((s - e[rows, y] - e[rows, drop]) / s))
        return dict(good, g=(c.T @ a + mu * x.reshape(k, n)).ravel())
    if kind == "missing - p (p.u)":
        p = RM.probabilities_f64(a, y, w, k, x)
        t = (w[:, None] * p) * (a @ v.reshape(k, n).T)
        q = (t.T @ a + mu * v.reshape(k, n)).ravel()
        return dict(good, q=q, c=float(v @ q))
    if kind == "mu added twice":
        return dict(good, g=good["g"] + mu * x, q=good["q"] + mu * v, c=good["c"] + mu * float(v @ v))
    if kind == "a masked row that leaks":
        w2 = np.where(w == 0.0, 1e-9, w)
        return _restated((a, y, w2, k, mu, None, v), x, "numpy")
    if kind == "a class block shifted by one":
        return dict(good, g=np.roll(good["g"], 1), q=np.roll(good["q"], 1))
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["wrong label column", "p_y - 1 with a dropped class", "missing - p (p.u)", "mu added twice", "a masked row that leaks",
                                  "a class block shifted by one"])
def test_planted_faults_are_rejected(kind):
    for (m, n, k) in [(64, 41, 17), (17, 7, 3)]:
        pr, x, truth = MC.truth_at(m, n, k, 1.0)
        assert np.any(pr[2] == 0.0)
        r = RM.ratios(_faulty(kind, pr, x), truth)
        assert max(r.values()) > 1.0, (kind, (m, n, k), r)


@pytest.mark.parametrize("m,n,k,ls", MC.CASES)
def test_newton_cg_windows_are_licensed(m, n, k, ls):
    w, worst, length = MC.licence(m, n, k, ls)
    ref, _, status = MC.ref_case(m, n, k, ls)
    print(f"multinomial NewtonCG {(m, n, k, ls)}: {ref.k} outer iterations ({status}), window {w} of {length}, worst disagreement {worst:.2e}")
    assert status == "ok" and ref.k <= MC.ITERS
    if (m, n, k) in MC.NEWTON_SHAPES:
        assert w >= MC.MIN_WINDOW and w >= length - 1, (w, length)
    else:
        assert w >= 3, (w, length)
    assert set(ref.why[:w]) <= {"tol", "cap"}


def test_negative_mu_meets_rule_4_at_once():
    ghg, gg = MC.neg_mu_curvature()
    assert ghg < 0.0 < gg
    ref = MC.run_ref(*MC.NEG_SHAPE, "bt", iters=3, mu=MC.NEG_MU)[0]
    assert ref.why[0] == "negcurv" and ref.inner[0] == 0


@pytest.mark.parametrize("kind,m,n,k", MC.FAMILY_CASES)
def test_family_windows_are_licensed(kind, m, n, k):
    _, w = MC.family_licence(kind, m, n, k)
    assert w >= 4, w


def test_k_2_is_the_logistic_objective():
    """with mu = 0 on both, f(W) = f_logistic(W_1 - W_0) and g_1 = -g_0 = g_logistic: the restatements agree to rounding"""
    import ref_logistic as RL
    a, y, w, k, _, x0, _ = MC.problem(17, 8, 2)
    f, g = RM.multinomial_fn(a, y, w, 2, 0.0)(x0)
    fl, gl = RL.logistic_fn(a, 2.0 * y - 1.0, w, 0.0)(x0[8:] - x0[:8])
    assert abs(f - fl) <= 1e-12 * abs(fl) and np.allclose(g[8:], gl, rtol=0, atol=1e-12) and np.allclose(g[:8], -gl, rtol=0, atol=1e-12)
