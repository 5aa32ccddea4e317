"""CPU: licenses the checker and the windows of tests/test_gpu_sparse_multinomial.py, and checks what needs no GPU.  The device's structure restated in
numpy (sparse_multinomial_cases.csr_functions: x to feature-major, a row pass over A, a column pass over the CSR of A', back to class-major) lies
inside ref_multinomial's derived bounds in three float64 summation orders; planted faults are each rejected by the same checker; every NewtonCG and
family window used on the GPU is licensed for the restatement alone and is at least MIN_WINDOW iterations or the whole run; the header declares the
four new entry points and the library exports them.  qn_csr_host.h gained no code: its stand-alone program (tests/csr_host_check.cpp) covers it.

SEED BASES: 4000 was the first base tried; the windows it gives are printed by test_every_newton_cg_window_is_licensed."""
import os
import re

import numpy as np
import pytest

import ref_multinomial as RM
import sparse_logistic_cases as SC
import sparse_multinomial_cases as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ("numpy", "fsum", "reversed")


# ---- 1. correct float64 evaluations lie inside the bounds ----
@pytest.mark.parametrize("m,n,k", SM.SHAPES)
def test_three_summation_orders_lie_inside_the_bounds(m, n, k):
    for scale in SM.SCALES:
        pr, x, truth = SM.truth_at(m, n, k, scale)
        for order in ORDERS:
            r = RM.ratios(SM.csr_eval(pr, x, pr["v"], order), truth)
            assert set(r) == {"f", "g", "p", "q", "c"} and max(r.values()) <= 1.0, (scale, order, r)


@pytest.mark.parametrize("m,n,k", [(3, 5, 3), (40, 65, 5), (96, 64, 16), (5, 2050, 4), (2050, 7, 3)])
def test_the_masked_cut_edges_and_unit_weights_lie_inside_the_bounds(m, n, k):
    for kind in ("unit", "edges"):
        pr, x, truth = SM.truth_at(m, n, k, 1.0, kind)
        r = RM.ratios(SM.csr_eval(pr, x, pr["v"]), truth)
        assert max(r.values()) <= 1.0, (kind, r)


def test_the_shapes_exercise_what_they_are_for():
    pr = SM.problem(40, 65, 5)
    lengths = np.diff(pr["indptr"])
    assert lengths[0] == 0 and lengths.max() == 64 and not pr["mask"][:, 64].any() and not np.any(pr["y"] == 4)
    assert SC.cut(SM.problem(5, 2050, 4)["indptr"])[2] == [2]
    pr = SM.problem(2050, 7, 3)
    g, _, longs = SC.cut(pr["indptr"])
    tptr = SC.transpose_csr(pr["indptr"], pr["indices"], pr["data"], 7)[0]
    assert g >= 2 and longs == [] and SC.cut(tptr)[2] == [0] and np.all(pr["a"][:, 0] == 1.0)  # the column of ones is a long row of A'
    pr = SM.problem(4096, 300, 4)
    tptr = SC.transpose_csr(pr["indptr"], pr["indices"], pr["data"], 300)[0]
    assert SC.cut(pr["indptr"])[0] > 256 and SC.cut(tptr)[0] > 256
    assert 16 * ((16 * 1025 + 15) // 16) > 16384 and 16 * 1024 == 16384  # one tile past what Multinomial takes
    assert 300 > 64 * SM.KR and 600 > 2 * 64 * SM.KR and 65 > 64 and 17 > 16  # past one class block, past two, a second slot, one past a full group
    assert 5 * 20000 == 100000 and np.all(np.diff(SM.problem(64, 20000, 5)["indptr"]) == 8)
    for shape in [(96, 64, 16), (2050, 7, 3), (4096, 300, 4)]:  # the masked rows sit at the first and the last row of a workgroup's cut
        base, edges = SM.problem(*shape), SM.problem(*shape, "edges")
        _, start, _ = SC.cut(base["indptr"])
        b = [b for b in range(len(start) - 1) if start[b + 1] > start[b]][-1]
        assert edges["w"][start[b]] == 0.0 and edges["w"][start[b + 1] - 1] == 0.0
    for shape in SM.SHAPES:
        if shape[0] >= 3:
            assert np.any(SM.problem(*shape)["w"] > 0.0)


def test_saturated_margins():
    pr, x, spread = SM.saturated_problem()
    truth = RM.truth_and_bound(pr["a"], pr["y"], pr["w"], pr["k"], pr["mu"], x)
    got = SM.csr_eval(pr, x)
    assert np.isfinite(got["f"]) and got["f"] > spread and max(RM.ratios(got, truth).values()) <= 1.0
    assert got["p"][0, 1] == 0.0 and got["p"][0, 0] == 1.0 and not got["p"][2].any()


# ---- 2. planted faults are rejected ----
def _drop(pr, keep, ptr):
    return dict(pr, indptr=ptr, indices=pr["indices"][keep], data=pr["data"][keep])


def _faulty(fault):
    """(what a device with the fault would return, the truth it is held against, the quantities of which at least one must leave its bound)"""
    if fault == "wrong_class_stride":  # W[k, j] taken from x[k (n + 1) + j]: class 0 is right, every other class is shifted
        pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
        k, n = 16, 64
        flat = np.concatenate([x, np.zeros(k)])
        wrong = np.array([[flat[c * (n + 1) + j] for j in range(n)] for c in range(k)]).ravel()
        got = SM.csr_eval(pr, wrong, pr["v"])
        return dict(got, g=got["g"] - pr["mu"] * wrong + pr["mu"] * x), truth, ("f", "g", "p")
    if fault == "last_entry_of_a_long_row_dropped":
        pr, x, truth = SM.truth_at(5, 2050, 4, 1.0, "unit")
        keep = np.ones(pr["data"].size, dtype=bool)
        keep[pr["indptr"][3] - 1] = False
        ptr = pr["indptr"].copy()
        ptr[3:] -= 1
        return SM.csr_eval(_drop(pr, keep, ptr), x, pr["v"]), truth, ("f", "g", "p", "q")
    if fault == "s_without_the_labelled_class":
        pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
        z = pr["a"] @ x.reshape(16, 64).T
        e = np.exp(z - z.max(axis=1)[:, None])
        rows = np.arange(96)
        sn = e.sum(axis=1) - e[rows, pr["y"]]
        p = np.where((pr["w"] != 0.0)[:, None], e / sn[:, None], 0.0)
        return dict(SM.csr_eval(pr, x, pr["v"]), p=p), truth, ("p",)
    if fault == "masked_row_leaking":
        pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
        w = pr["w"].copy()
        w[int(np.argmax(w == 0.0))] = 1.0
        return SM.csr_eval(dict(pr, w=w), x, pr["v"]), truth, ("f", "g", "p")
    if fault == "mu_missing_from_q":
        pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
        got = SM.csr_eval(pr, x, pr["v"])
        return dict(got, q=got["q"] - pr["mu"] * pr["v"]), truth, ("q",)
    if fault == "feature_major_vector_returned":
        pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
        got = SM.csr_eval(pr, x, pr["v"])
        return dict(got, g=np.ascontiguousarray(got["g"].reshape(16, 64).T).ravel()), truth, ("g",)
    if fault == "p_from_the_trial_point":
        pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
        return SM.csr_eval(pr, x, pr["v"], p_at=1.25 * x), truth, ("q", "c")
    if fault == "transpose_with_two_values_swapped":
        pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
        tptr, tidx, tdata = SC.transpose_csr(pr["indptr"], pr["indices"], pr["data"], 64)
        live = pr["w"] > 0.0
        j = next(j for j in range(64) if tptr[j + 1] - tptr[j] >= 2 and live[tidx[tptr[j]]] and live[tidx[tptr[j] + 1]])
        tdata = tdata.copy()
        tdata[tptr[j]], tdata[tptr[j] + 1] = tdata[tptr[j] + 1], tdata[tptr[j]]
        return SM.csr_eval(pr, x, pr["v"], t=(tptr, tidx, tdata)), truth, ("g", "q")
    pr, x, truth = SM.truth_at(96, 64, 16, 1.0)
    return SM.csr_eval(pr, x, pr["v"]), truth, ()


FAULTS = ["wrong_class_stride", "last_entry_of_a_long_row_dropped", "s_without_the_labelled_class", "masked_row_leaking", "mu_missing_from_q",
          "feature_major_vector_returned", "p_from_the_trial_point", "transpose_with_two_values_swapped"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_rejected(fault):
    got, truth, _ = _faulty("none")
    assert max(RM.ratios(got, truth).values()) <= 1.0  # (the same code without a fault passes)
    got, truth, must = _faulty(fault)
    r = RM.ratios(got, truth)
    assert any(r[key] > 1.0 for key in must), (fault, r)


# ---- 3. the windows ----
@pytest.mark.parametrize("m,n,k,ls", SM.CASES)
def test_every_newton_cg_window_is_licensed(m, n, k, ls):
    """a window may stop early, never below MIN_WINDOW; where the run converges sooner it is the whole run (but the iteration that finds it converged)"""
    w, worst, length = SM.licence(m, n, k, ls)
    s, _, status = SM.ref_case(m, n, k, ls)
    print(f"sparse multinomial NewtonCG {(m, n, k, ls)}: window {w} of {length}, worst disagreement inside {worst:.2e}, inner {s.inner}")
    assert status == "ok" and w >= 1 and (w >= SM.MIN_WINDOW or w >= length - 1), (w, length, status)
    pr = SM.problem(m, n, k)
    g = RM.truth_and_bound(pr["a"], pr["y"], pr["w"], k, pr["mu"], s.x)["g"]
    assert float(np.max(np.abs(g))) < SM.TOL  # the restatement converges to 1e-7 on every chosen shape, under both searches


def test_negative_mu_reaches_rule_4_at_j_0():
    ghg, gg = SM.neg_mu_curvature()
    assert ghg < 0.0 < gg
    s = SM.run_ref(*SM.NEG_SHAPE, "bt", iters=3, mu=SM.NEG_MU)[0]
    assert s.why[0] == "negcurv" and s.inner[0] == 0


@pytest.mark.parametrize("kind,m,n,k", SM.FAMILY_CASES)
def test_family_windows_are_licensed(kind, m, n, k):
    ref, w = SM.family_licence(kind, m, n, k)
    print(f"sparse multinomial {kind} {(m, n, k)}: window {w} of {len(ref.trace)}")
    assert w >= 4, (w, len(ref.trace))


# ---- 4. the boundary ----
NEW_ENTRY_POINTS = ("qn_sparse_multinomial_create", "qn_sparse_multinomial_info", "qn_sparse_multinomial_set_lanes", "qn_sparse_multinomial_probabilities")


def test_the_header_declares_and_the_library_exports_the_new_entry_points(qn):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qn_hip.h")).read(), flags=re.S)
    lib = qn._abi.lib()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert hasattr(lib, name), name
    assert lib.qn_abi_version() == 5
    for attr in ("from_scipy", "set_lanes", "probabilities", "lanes", "n_long_rows", "n_long_cols", "nnz", "kp"):
        assert hasattr(qn.SparseMultinomial, attr), attr
    # the refusals that need no device: an objective handle is never reached
    assert lib.qn_sparse_multinomial_set_lanes(None, 0, 0) == 3 and lib.qn_sparse_multinomial_info(None, None, None, None, None, None, None) == 3
    assert lib.qn_sparse_multinomial_probabilities(None, None, None) == 3


def test_the_padding_rule_and_the_automatic_lanes():
    assert [SM.kp(k) for k in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 300, 600)] == [2, 4, 4, 8, 8, 16, 16, 32, 32, 48, 64, 80, 304, 608]
    assert SM.auto_lanes(1 << 20, 16 << 20, 4) == 4 and SM.auto_lanes(1 << 20, 16 << 20, 16) == 1 and SM.auto_lanes(1 << 20, 16 << 20, 64) == 1
    assert SM.auto_lanes(1 << 20, 16 << 20, 2) == 8 and SM.auto_lanes(100, 300, 2) == 1
