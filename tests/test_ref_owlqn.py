"""CPU tests of tests/ref_owlqn.py, the restatement the GPU solver QN_OWLQN is checked against: with l1 = 0 it IS
ref_lbfgs.LBFGS + BackTracking; on separable quadratics it ends at the closed-form minimiser with exact zeros; the windows
tests/test_gpu_owlqn.py compares are the ones over which three summation orders and two formulations of H_k v take the same decisions; the whole
runs reach ref_prox.SpectralProximalGradient's zero pattern and x; seven planted faults are each rejected by a comparison the suites make; and
tests/owlqn_replay.py is licensed on the float64 restatement."""
import numpy as np
import pytest

import lbfgs_cases as LBC
import owlqn_cases as OC
import owlqn_replay as OR
import ref_lbfgs as RL
import ref_owlqn as RO
import ref_spg as R


def test_l1_zero_is_lbfgs():
    """no penalty: v = g, nothing is aligned away or projected; t, x and the counts are ref_lbfgs.LBFGS's bit for bit (its Armijo right side
    c1 t g.d against c1 g.(xt - x) differs by rounding only: same decisions on this case, checked)"""
    n, iters = 64, 25
    fn, x0 = LBC.oracle_fn("host", n)
    lb, ub = LBC.free_box(n)
    a, _, _ = LBC.run_ref(fn, x0, lb, ub, "bt", 5, iters)
    o = R.CountingOracle(fn)
    s = RO.OWLQN(LBC.TOL, x0, 0.0, m=5)
    with pytest.raises(R.MaxIterReached):
        s.minimize(OC.line_search(), o, iters, 50)
    assert len(a.trace) == len(s.trace) == iters
    for k in range(iters):
        for key in ("gnorm", "t", "n_evals", "ls_iters", "s_norm"):
            assert a.trace[k][key] == s.trace[k][key], (k, key)
        assert a.trace_x[k].tobytes() == s.trace_x[k].tobytes(), k
    assert a.updated == s.updated


def test_closed_form_separable_quadratic():
    """f = 1/2 sum q_j (x_j - c_j)^2: the minimiser of f + h is soft(c_j, l1_j / q_j), entry by entry; see tests/test_ref_prox.py for the bound.
    (tol 1e-5: the monotone search compares composite values and stalls once a step's decrease is below F's last bit -- here F = 1073.7 and the
    run stops moving at a measure of 1.6e-6 --)"""
    n, tol = 200, 1e-5
    rng = np.random.default_rng(11)
    q, c, l1 = rng.uniform(1.0, 50.0, n), rng.standard_normal(n), rng.uniform(0.0, 30.0, n)
    l1[::9] = 0.0

    def fn(x):
        return 0.5 * float(np.sum(q * (x - c) ** 2)), q * (x - c)
    want = np.sign(c) * np.maximum(np.abs(c) - l1 / q, 0.0)
    must_be_zero = np.abs(c) * q < l1 - 1e-6
    assert 20 < must_be_zero.sum() < n - 20
    o = R.CountingOracle(fn)
    s = RO.OWLQN(tol, rng.standard_normal(n), l1)
    s.minimize(OC.line_search(), o, 2000, 50)  # returns: converged
    assert s.has_converged(fn(s.x))
    assert np.all(s.x[must_be_zero] == 0.0) and not np.any(np.signbit(s.x[s.x == 0.0]))
    assert np.max(np.abs(s.x - want)) <= tol / q.min()


def test_element_rules_on_crafted_entries():
    x = np.array([0.0, 0.0, 0.0, 1.0, -1.0, 0.5, 0.0])
    g = np.array([0.2, -0.9, 0.9, -0.5, 0.2, -3.0, 0.3])
    l1 = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.0, 0.0])
    v = RO.pseudo_gradient(x, g, l1)
    assert np.array_equal(v, [0.0, -0.4, 0.4, 0.0, -0.3, -3.0, 0.3])
    z = np.array([1.0, 2.0, 2.0, 1.0, -1.0, 4.0, -1.0])  # entry 1: z against v; entry 6: smooth, z against v all the same
    d = RO.align(z, v, l1)
    assert np.array_equal(d, [0.0, 0.0, -2.0, 0.0, 1.0, -4.0, 1.0]) and not np.any(np.signbit(d[d == 0.0]))
    xt = RO.project(x, np.array([0.0, 1.0, 1.0, -3.0, 0.5, -1.0, -2.0]), v, l1, 1.0)
    # entry 1 leaves along -v; entry 2 would leave against -v: stays; entry 3 crosses zero: 0.0; entry 5 is smooth and crosses freely
    assert np.array_equal(xt, [0.0, 1.0, 0.0, 0.0, -0.5, -0.5, -2.0]) and not np.any(np.signbit(xt[xt == 0.0]))


@pytest.mark.parametrize("kind,shape,m", OC.WINDOW_CASES)
def test_window_self_check(qo, kind, shape, m):
    w = OC.window(kind, shape, m, qo)
    assert w == OC.WINDOWS[(kind, shape, m)], w
    assert w >= 20
    a = OC.run_ref(kind, shape, m, qo)[0]
    assert 0 < np.count_nonzero(a.x) < a.x.size  # the penalty bites: exact zeros and live entries
    assert any(r["ls_iters"] > 1 for r in a.trace[:w])  # a backtracking step is inside the window
    assert sum(a.updated[:w]) > m  # the ring wraps inside the window
    print(f"window {kind} {shape} m={m}: {w}, nonzeros {np.count_nonzero(a.x)} of {a.x.size}")


def test_whole_runs_reach_the_proximal_solver_s_answer():
    assert OC.run_tol() == OC.RUN_TOL
    gap = OC.run_gap()
    print(f"RUN_TOL {OC.RUN_TOL:g}, largest |x_owlqn - x_prox| {gap!r}")
    assert gap == OC.RUN_GAP
    for case in OC.RUN_CASES:
        s, status = OC.run_whole(*case)
        p, pstatus = OC.run_whole_prox(*case)
        assert status == pstatus == "ok", case
        assert 0 < np.count_nonzero(s.x) < case[2], case
        assert np.array_equal(s.x != 0.0, p.x != 0.0), case
        assert s.x[0] != 0.0  # the unpenalised column
        for order in ("fsum", "reversed"):
            o, ostatus = OC.run_whole(*case, order=order)
            assert ostatus == "ok" and np.array_equal(o.x != 0.0, s.x != 0.0), (case, order)


# ---- planted faults: each wrong rule is rejected by a comparison these tests and the GPU tests make ----
def _windows_rejecting(qo, fault):
    out = []
    for c in OC.WINDOW_CASES:
        clean = OC.run_ref(*c, qo=qo)[0]
        bad = OC.run_ref(*c, qo=qo, faults=(fault,))[0]
        if OC.agree(clean, bad, OC.WINDOWS[c]) is not None:
            out.append(c)
    return out


@pytest.mark.parametrize("fault", ["pg_at_zero_is_g", "no_alignment", "orthant_from_x", "accept_unprojected", "y_from_pseudo"])
def test_planted_fault_breaks_every_window(qo, fault):
    """the window comparison (equal counts, t and x to 1e-9, the measure to 1e-7) against the clean restatement"""
    assert _windows_rejecting(qo, fault) == OC.WINDOW_CASES, fault


def test_planted_fault_no_exemption_breaks_the_windows_with_smooth_entries(qo):
    broken = _windows_rejecting(qo, "no_exemption")
    assert broken == [c for c in OC.WINDOW_CASES if np.ndim(OC.l1_of(c[0], c[1])) == 1], broken


def test_planted_faults_change_the_element_rules():
    """... and the bit-for-bit element checks of tests/test_gpu_owlqn.py"""
    x, g, l1 = np.array([0.0, 0.0, 1.0]), np.array([0.2, -0.9, -0.5]), np.array([0.5, 0.5, 0.5])
    assert RO.pseudo_gradient(x, g, l1).tobytes() != RO.pseudo_gradient(x, g, l1, faults=("pg_at_zero_is_g",)).tobytes()
    z, v = np.array([1.0, -1.0]), np.array([-0.5, -0.5])
    assert np.array_equal(RO.align(z, v, l1[:2]), [0.0, 1.0]) and np.array_equal(RO.align(z, v, l1[:2], faults=("no_alignment",)), [-1.0, 1.0])
    assert np.array_equal(RO.align(z, v, np.zeros(2)), [-1.0, 1.0]) and np.array_equal(RO.align(z, v, np.zeros(2), faults=("no_exemption",)), [0.0, 1.0])
    x0, d0, v0 = np.array([0.0]), np.array([1.0]), np.array([-1.0])
    assert RO.project(x0, d0, v0, l1[:1], 1.0)[0] == 1.0 and RO.project(x0, d0, v0, l1[:1], 1.0, faults=("orthant_from_x",))[0] == 0.0


@pytest.mark.parametrize("n", [1, 2])
def test_planted_fault_armijo_right_side(n):
    """c1 t v.d in place of c1 v.(xt - x): on owlqn_cases.tiny_problem the first search halves instead of accepting t = 1 -- the run
    tests/test_gpu_owlqn.py::test_tiny_first_iteration_bit_for_bit compares bit for bit"""
    clean, bad = OC.run_tiny(n), OC.run_tiny(n, faults=("armijo_t_vd",))
    assert clean.trace[0]["ls_iters"] == 1 and clean.trace[0]["t"] == 1.0 and clean.trace_x[0][0] == 0.0
    assert bad.trace[0]["ls_iters"] > 1 and bad.trace[0]["t"] < 1.0


def test_every_fault_is_covered():
    assert set(RO.FAULTS) == {"pg_at_zero_is_g", "no_alignment", "orthant_from_x", "accept_unprojected", "y_from_pseudo", "armijo_t_vd", "no_exemption"}


def test_state_across_calls_and_set_l1():
    """rule 9 on the restatement: two calls of k iterations are one call of 2 k; set_l1 keeps the pairs; set_memory drops them"""
    _, fn, x0 = OC.restart_problem()
    k = OC.RESTART_K

    def run(calls, iters):
        o = R.CountingOracle(fn)
        s = RO.OWLQN(OC.TOL, x0, OC.RESTART_L1[0])
        xs = []
        for _ in range(calls):
            with pytest.raises(R.MaxIterReached):
                s.minimize(OC.line_search(), o, iters, OC.MAX_LS)
            xs += s.trace_x
        return s, xs
    one, xs1 = run(1, 2 * k)
    two, xs2 = run(2, k)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(xs1, xs2)) and len(xs1) == len(xs2) == 2 * k
    stored = two.stored_pairs()
    assert stored == 5
    two.set_l1(OC.RESTART_L1[1])
    assert two.stored_pairs() == stored
    two.set_memory(3)
    assert two.stored_pairs() == 0


# ---- the replay checker, licensed on the float64 restatement ----
@pytest.mark.parametrize("case", OC.REPLAY_CASES, ids=[c["name"] for c in OC.REPLAY_CASES])
def test_replay_is_licensed_on_the_restatement(case):
    run = OC.replay_ref(case)
    assert len(run.xs) == case["iters"] * case["calls"]
    rep = OR.replay(run)
    OR.check(rep, case["name"])
    assert rep.commits > case["m"] and rep.head_advances > 0  # the ring wraps
    if case["m"] == 32:
        assert rep.max_k == 32
    assert 0 < np.count_nonzero(run.xs[-1]) < case["n"]


def test_replay_rejects_planted_faults():
    """the replay tells a wrong run from a right one: a restatement with each direction- or point-forming fault fails it"""
    import owlqn_cases as C
    case = next(c for c in C.REPLAY_CASES if c["name"] == "wrap-m5-n2050")
    fn, x0, l1 = C.replay_problem(case)
    for fault in ("no_alignment", "accept_unprojected", "y_from_pseudo", "orthant_from_x"):
        rec = OR.Recorder(fn)
        o = R.CountingOracle(rec)
        s = RO.OWLQN(C.REPLAY_TOL, x0, l1, m=case["m"], faults=(fault,))
        run = OR.Run(case["m"], False, l1, x0, rec)
        states = []
        try:
            s.minimize(C.line_search(), o, case["iters"], C.MAX_LS, callback=lambda r: states.append((r.stored_pairs(), r.gamma, r.resets)))
        except (R.MaxIterReached, RO.AbnormalTermination):
            pass
        run.extend(s.trace_x, [r["t"] for r in s.trace], s.updated, states)
        rep = OR.replay(run)
        bad = [k for k, (r, a) in enumerate(zip(rep.ratios, rep.asserted)) if a and not r <= 1.0]
        assert bad or rep.problems, fault
