"""CPU: licenses the checker and the windows of tests/test_gpu_logistic.py.  Three float64 summation orders of ref_logistic.logistic_fn and of the
Hessian-vector product lie inside the derived bounds at every shape and scale; planted faults are each rejected by the same checker; every NewtonCG
window is at least MIN_WINDOW iterations or the whole run; the convergence shapes reach 1e-7; the restatement's gradient agrees with a longdouble
central difference of its f."""
import numpy as np
import pytest

import cg_cases as C
import logistic_cases as LC
import ref_logistic as RL

LD = np.longdouble
ORDERS = ("numpy", "fsum", "reversed")


def _eval(a, y, w, mu, x, v, dot):
    f, g = RL.logistic_fn(a, y, w, mu, dot)(x)
    q = RL.logistic_hess_vec_at(a, y, w, mu, dot)(x)(v)
    return dict(f=f, g=g, d=RL.weights_f64(a, y, w, x, dot), q=q, c=float(np.dot(v, q) if dot is None else dot(v, q)))


def _worst(got, truth):
    r = RL.ratios(got, truth)
    return max(r.values()), r


# ---- 1. a correct float64 evaluation lies inside the bounds ----
@pytest.mark.parametrize("scale", LC.SCALES)
@pytest.mark.parametrize("m,n", LC.SHAPES)
def test_three_summation_orders_lie_inside_the_bounds(m, n, scale):
    (a, y, w, mu, _, v), x, truth = LC.truth_at(m, n, scale)
    for order in ORDERS:
        worst, r = _worst(_eval(a, y, w, mu, x, v, None if order == "numpy" else C.DOTS[order]), truth)
        assert worst <= 1.0, (order, r)


def test_unit_weights_and_masked_cut_edges_lie_inside_the_bounds():
    for kind in ("unit", "edges"):
        for (m, n) in [(96, 64), (40, 65), (257, 200)]:
            (a, y, w, mu, _, v), x, truth = LC.truth_at(m, n, 1.0, kind)
            assert _worst(_eval(a, y, w, mu, x, v, None), truth)[0] <= 1.0
            if kind == "edges":
                _, per = LC.row_cut(m)
                assert w[per] == 0.0 and w[min(m, 2 * per) - 1] == 0.0 and np.all(np.asarray(truth["d"])[w == 0.0] == 0)


# ---- 2. planted faults are rejected ----
def _faulty(fault, a, y, w, mu, x, v):
    yw = y * w
    u = a @ x
    l, coef, d, s = RL.row_terms(yw, u)
    k = int(np.argmax((w > 0.0) & (y < 0.0)))  # a live row with the label -1
    if fault == "label_sign_ignored_on_one_row":
        lk, ck, dk, _ = RL.row_terms(np.array([-yw[k]]), np.array([u[k]]))  # (the other label's loss and slope)
        l[k], coef[k], d[k] = lk[0], -ck[0], dk[0]  # (z = +u where the label says -u: the coefficient keeps yw's sign, s is the wrong one)
    elif fault == "masked_row_counted":
        j = int(np.argmax(w == 0.0))
        lj, cj, dj, _ = RL.row_terms(np.array([y[j]]), np.array([u[j]]))
        l[j], coef[j], d[j] = lj[0], cj[0], dj[0]
    elif fault == "weight_dropped_from_d":
        d = np.where(w > 0.0, d / np.where(w > 0.0, w, 1.0), 0.0)
    elif fault == "last_row_of_a_cut_dropped":
        _, per = LC.row_cut(a.shape[0])
        live = [r for r in range(per - 1, a.shape[0], per) if w[r] > 0.0]
        l[live[0]] = coef[live[0]] = d[live[0]] = 0.0
    elif fault == "s_off_by_16_ulp":
        s16 = s + 16.0 * np.spacing(s)
        coef = np.where(yw != 0.0, -(yw * s16), 0.0)
    mux = 0.0 * x if fault == "mu_x_omitted" else mu * x
    f = float(np.sum(l)) + 0.5 * mu * float(x @ x)
    g = a.T @ coef + mux
    q = a.T @ (d * (a @ v)) + mu * v
    return dict(f=f, g=g, d=d, q=q, c=float(v @ q))


FAULTS = {  # fault: the quantities of which at least one must leave its bound
    "label_sign_ignored_on_one_row": ("f", "g"),
    "masked_row_counted": ("f", "g", "d"),
    "weight_dropped_from_d": ("d", "q"),
    "mu_x_omitted": ("g",),
    "last_row_of_a_cut_dropped": ("f", "g", "d"),
    "s_off_by_16_ulp": ("g",),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_rejected(fault):
    if fault == "s_off_by_16_ulp":
        # 16 ulp of s against the C = 8 cap shows where nothing else is large: one row (gamma_(m+2) = 3 u), a small margin (dz of 3 u |a x|) -- the bound on
        # g is then about 12 u |a| w s, and 16 ulp of s are 16 to 32 u s
        (a, y, w, mu, _, v), x, truth = LC.truth_at(1, 1, 1e-3, "unit")
    else:
        (a, y, w, mu, _, v), x, truth = LC.truth_at(96, 64, 1.0)
        assert np.any(w == 0.0) and np.any((w != 1.0) & (w > 0.0)) and np.any((w > 0.0) & (y < 0.0))
    assert _worst(_faulty("none", a, y, w, mu, x, v), truth)[0] <= 1.0  # (the same code without a fault passes)
    r = RL.ratios(_faulty(fault, a, y, w, mu, x, v), truth)
    assert any(r[key] > 1.0 for key in FAULTS[fault]), (fault, r)


def test_the_unstable_log_is_rejected_at_a_margin_of_minus_800():
    a, y, w, mu, x, z = LC.saturated_problem()
    truth = RL.truth_and_bound(a, y, w, mu, x)
    f, g = RL.logistic_fn(a, y, w, mu)(x)
    d = RL.weights_f64(a, y, w, x)
    assert np.isfinite(f) and RL.ratios(dict(f=f, g=g, d=d), truth)["f"] <= 1.0
    assert d[0] == 0.0 and d[1] == 0.0 and d[2] == 0.0 and d[3] > 0.0 and g[1] == mu * x[1]  # (s = d = 0 exactly on the saturated side)
    with np.errstate(over="ignore"):
        unstable = float(np.sum(w * np.log(1.0 + np.exp(-z)))) + 0.5 * mu * float(x @ x)
    assert not RL.ratios(dict(f=unstable), truth)["f"] <= 1.0


# ---- 3. the windows ----
@pytest.mark.parametrize("m,n,ls", LC.CASES)
def test_every_window_is_min_window_or_the_whole_run(m, n, ls):
    w, worst, length = LC.licence(m, n, ls)
    print(f"logistic NewtonCG {(m, n, ls)}: window {w} of {length}, worst disagreement inside {worst:.2e}, inner {LC.ref_case(m, n, ls)[0].inner}")
    assert w >= min(LC.MIN_WINDOW, length - 1) and w >= 1, (w, length)
    assert w >= LC.MIN_WINDOW or w >= length - 1


@pytest.mark.parametrize("m,n", LC.CONVERGENCE)
def test_convergence_shapes_reach_the_tolerance(m, n):
    for ls in LC.SEARCHES:
        s, _, status = LC.ref_case(m, n, ls)
        a, y, w, mu, _, _ = LC.problem(m, n)
        g = RL.truth_and_bound(a, y, w, mu, s.x)["g"]
        assert status == "ok" and float(np.max(np.abs(g))) < LC.TOL, (ls, status)


def test_negative_mu_reaches_rule_4_at_j_0():
    ghg, gg = LC.neg_mu_curvature()
    assert ghg < 0.0 < gg
    s = LC.run_ref(3, 5, "bt", iters=3, mu=LC.NEG_MU)[0]
    assert s.why[0] == "negcurv" and s.inner[0] == 0


@pytest.mark.parametrize("kind,m,n", LC.FAMILY_CASES)
def test_family_windows_are_licensed(kind, m, n):
    ref, w = LC.family_licence(kind, m, n)
    print(f"logistic {kind} {(m, n)}: window {w} of {len(ref.trace)}")
    assert w >= 4, (w, len(ref.trace))


# ---- 4. the restatement itself ----
def test_gradient_agrees_with_a_longdouble_central_difference():
    a, y, w, mu, x0, _ = LC.problem(3, 5)
    assert np.any(w > 0.0)
    g = RL.logistic_fn(a, y, w, mu)(x0)[1]
    h = LD(2.0) ** -24
    for j in range(5):
        e = np.zeros(5, dtype=LD)
        e[j] = h
        fp = RL.truth_and_bound(a, y, w, mu, x0.astype(LD) + e)["f"]
        fm = RL.truth_and_bound(a, y, w, mu, x0.astype(LD) - e)["f"]
        assert abs(float((fp - fm) / (2 * h)) - g[j]) <= 1e-9 * max(1.0, abs(g[j])), j
