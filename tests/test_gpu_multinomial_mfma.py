"""GPU tests of the multinomial objective's second stream kernel, mnl_mfma_kernel (v_mfma_f64_16x16x4_f64; `Multinomial.set_kernel(2)`): the same
derived bounds of tests/ref_multinomial.py as the register-blocked kernel is held to, at the same shapes (all have K <= 64) and at one shape with two
16-row tiles in a workgroup's cut, repeatable bits, the switch back to the other kernel, the refusal where the kernel is not built, and NewtonCG inside
the licensed windows with the product in this kernel."""
import numpy as np
import pytest

import multinomial_cases as MC
import ref_multinomial as RM
from test_gpu_multinomial import _check_point, _obj, newton_run

pytestmark = pytest.mark.gpu
MFMA = 2
# (4200, 5, 3): per = 17 rows in a workgroup's cut -- a full tile of 16 rows and a tile of one
SHAPES = MC.SHAPES + [(4200, 5, 3)]


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_everything_inside_the_bounds_mfma(qn, m, n, k):
    for kind, scales in (("weighted", MC.SCALES), ("unit", [1.0]), ("edges", [1.0]), ("absent", [1.0])):
        obj = None
        try:
            for scale in scales:
                pr, x, truth = MC.truth_at(m, n, k, scale, kind)
                obj = obj or _obj(qn, pr, kernel=MFMA)
                _check_point(obj, pr, x, truth, f"mfma {(m, n, k)} {kind} scale {scale:g}")
        finally:
            if obj:
                obj.close()


@pytest.mark.parametrize("m,n,k", [(17, 7, 3), (1031, 12, 4)])
def test_a_masked_row_whose_margins_overflow_mfma(qn, m, n, k):
    pr = MC.variant(m, n, k, "overflow")
    x = MC.overflow_point(pr)
    tame = pr[0].copy()
    tame[m // 2, :] = 0.0
    obj, ref = _obj(qn, pr, kernel=MFMA), qn.Multinomial(tame, pr[1], k, pr[4], weights=pr[2])
    try:
        ref.set_kernel(MFMA)
        ev, ev2 = obj(x), ref(x)
        (q, c), (q2, c2) = obj.hess_vec_at(x, pr[6]), ref.hess_vec_at(x, pr[6])
        p = obj.probabilities(x)
        assert np.isfinite(ev.f()) and np.all(np.isfinite(ev.g())) and np.all(np.isfinite(q)) and np.isfinite(c) and np.all(np.isfinite(p))
        assert ev.f() == ev2.f() and ev.g().tobytes() == ev2.g().tobytes() and q.tobytes() == q2.tobytes() and c == c2
        assert np.all(p[m // 2] == 0.0)
    finally:
        obj.close()
        ref.close()


def test_same_bits_and_the_switch_between_the_kernels(qn):
    for (m, n, k) in [(17, 8, 16), (64, 41, 17), (20, 256, 64)]:
        pr, x, _ = MC.truth_at(m, n, k, 1.0)
        one, two = _obj(qn, pr), _obj(qn, pr)
        try:
            v1 = one(x)
            vq, vc = one.hess_vec_at(x, pr[6])
            one.set_kernel(MFMA)
            two.set_kernel(MFMA)
            a1, a2, b1 = one(x), one(x), two(x)
            assert a1.f() == a2.f() == b1.f() and a1.g().tobytes() == a2.g().tobytes() == b1.g().tobytes()
            (q1, c1), (q2, c2), (q3, c3) = one.hess_vec_at(x, pr[6]), one.hess_vec_at(x, pr[6]), two.hess_vec_at(x, pr[6])
            assert q1.tobytes() == q2.tobytes() == q3.tobytes() and c1 == c2 == c3
            assert one.probabilities(x).tobytes() == two.probabilities(x).tobytes()
            # back to the register-blocked kernel: its bits; the automatic choice, which a new object has: the MFMA kernel above 16 classes
            fresh = qn.Multinomial(pr[0], pr[1], k, pr[4], weights=pr[2])
            try:
                for back, (ef, eg, eq, ec) in ((1, (v1.f(), v1.g(), vq, vc)), (0, (a1.f(), a1.g(), q1, c1) if k > 16 else (v1.f(), v1.g(), vq, vc))):
                    one.set_kernel(back)
                    for o in (one, fresh) if back == 0 else (one,):
                        v2 = o(x)
                        assert v2.f() == ef and v2.g().tobytes() == eg.tobytes(), (k, back)
                        q4, c4 = o.hess_vec_at(x, pr[6])
                        assert q4.tobytes() == eq.tobytes() and c4 == ec, (k, back)
            finally:
                fresh.close()
        finally:
            one.close()
            two.close()


def test_set_kernel_refusals(qn):
    pr, x, truth = MC.truth_at(9, 60, 200, 1.0)
    obj = _obj(qn, pr)
    try:
        with pytest.raises(qn.ErrorInputParams, match="MFMA kernel is not built for this shape"):
            obj.set_kernel(MFMA)
        for bad in (-1, 3):
            with pytest.raises(qn.ErrorInputParams, match="kernel must be 0"):
                obj.set_kernel(bad)
        _check_point(obj, pr, x, truth, "(9, 60, 200) after the refused switch")  # (nothing changed)
    finally:
        obj.close()


@pytest.mark.parametrize("m,n,k,ls", [(96, 16, 4, "bt"), (64, 41, 17, "wolfe")])
def test_newton_cg_against_the_restatement_mfma(qn, m, n, k, ls):
    w = MC.window(m, n, k, ls)
    ref, _, ref_status = MC.ref_case(m, n, k, ls)
    run = newton_run(qn, m, n, k, ls, kernel=MFMA)
    assert len(run["trace"]) >= w
    for i in range(w):
        r, g = ref.trace[i], run["trace"][i]
        dx = float(np.linalg.norm(run["xs"][i] - ref.trace_x[i]) / max(1.0, np.linalg.norm(ref.trace_x[i])))
        assert dx <= MC.GPU_TOL, (i, dx)
        assert g["n_evals"] == r["n_evals"] and g["ls_iters"] == r["ls_iters"], (i, g, r)
        assert run["inner"][i] == ref.inner[i], (i, run["inner"], ref.inner)
    assert run["status"] == "ok" and ref_status == "ok" and run["k"] == ref.k, (run["k"], ref.k, run["status"])
    pr = MC.problem(m, n, k)
    g = RM.truth_and_bound(pr[0], pr[1], pr[2], k, pr[4], run["x"])["g"]
    assert float(np.max(np.abs(g))) < MC.TOL
