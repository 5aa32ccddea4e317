"""GPU tests of Newton on the device log-sum-exp objective: the MFMA f64 Hessian kernel (csrc/qn_lse_hess.hip.h) against an extended-precision
evaluation inside the derived bound of DESIGN.md 20, its structure (bitwise symmetry, bitwise repeatability), and whole Newton runs -- Cholesky
and pivoted LU -- against the oracle's run (licensed on the CPU by tests/test_ref_newton_lse.py) and the host-closure GPU run of the same problem.

The tolerance on x of the Newton runs: the host-closure GPU path -- same solver, same factorisation, the Hessian from numpy -- was run against the oracle
before the device path existed; HOST_DIST holds its distance ||x - x_oracle|| per case.  The device path is allowed 8 times that, with the floor
n * 2^-52 * max(1, ||x||).  The two paths differ in the Hessian's summation order only, which the entrywise bound on the Hessian holds far below what the
factorisation contributes."""
import numpy as np
import pytest

import newton_lse_cases as NC
import pnewton_cases as PC

pytestmark = pytest.mark.gpu

# ||x_host_closure_gpu - x_oracle|| measured on the MI355X, (m, n, line search, memoize, pivoted LU) -> distance
HOST_DIST = {
    (96, 64, "mt", 0, 0): 4.205e-16,  # k 10, t0 1.0
    (96, 64, "mt", 1, 0): 4.205e-16,
    (96, 64, "bt", 0, 0): 4.073e-16,  # k 10, t0 1.0
    (96, 64, "bt", 1, 0): 4.073e-16,
    (257, 200, "mt", 0, 0): 5.047e-16,  # k 12, t0 0.2932797873471644 (oracle) / 0.29327978734716453 (host closure on the GPU)
    (257, 200, "mt", 1, 0): 5.047e-16,
    (257, 200, "bt", 0, 0): 4.803e-16,  # k 10, t0 0.5
    (257, 200, "bt", 1, 0): 4.803e-16,
    (96, 64, "mt", 1, 1): 4.205e-16,
    (96, 64, "bt", 1, 1): 4.073e-16,
}  # (8 times these is below the floor n * 2^-52 * max(1, ||x||) = 1.4e-14 / 4.6e-14 on every case: the floor is what binds)
# The first iteration's t.  A backtracking step is a power of beta and an accepted unit step is 1.0: those are compared for equality, on all
# three runs.  On (257, 200) More-Thuente INTERPOLATES the first step -- a rational function of f and g'd at the trial points, which the
# oracle, numpy and the device sum in three different orders -- and bitwise equality does not hold even between the two runs that are older
# than the device path.  Measured on the MI355X, in units of the last place of the oracle's t = 0.2932797873471644 (5.55e-17):
T_INTERP_ULPS_MEASURED = {
    "host": 2,      # host closure on the GPU: 0.29327978734716453
    "device": 348,  # device log-sum-exp:      0.29327978734718374 (1.93e-14 absolute, 6.6e-14 relative)
}
# allowed: the host-closure run 8 units (a few units in the last place: its f and g come from numpy on whatever CPU runs the test), the device
# run 8 times what it measured, as the distances above.
T_INTERP_ULPS_ALLOWED = {"host": 8, "device": 8 * T_INTERP_ULPS_MEASURED["device"]}


def _t_equal(t, t_ref, lsname, which):
    if lsname == "bt" or t_ref == 1.0:
        return t == t_ref
    return abs(t - t_ref) <= T_INTERP_ULPS_ALLOWED[which] * np.spacing(t_ref)


_dev = {}


def _device_hessians(qn, m, n, scale):
    """two calls of obj.hessian at scale * x0, once per case"""
    key = (m, n, scale)
    if key not in _dev:
        a, c, mu, x0 = NC.problem(m, n)
        obj = qn.LogSumExp(a, c, mu)
        _dev[key] = (obj.hessian(scale * x0), obj.hessian(scale * x0))
        obj.close()
    return _dev[key]


def _check_inside_bound(h, truth, bound, s, label):
    err = np.abs(h.astype(np.longdouble) - truth)
    units = float(np.max(err / (s * 2.0 ** -53)))
    print(f"{label}: max error {units:.2f} units of 2^-53 S_ij (bound {float(np.max(bound / s)) * 2.0 ** 53:.0f} units)")
    assert np.all(np.isfinite(h))
    assert np.all(err <= bound), (label, units)


SCALES = (1.0, NC.SPREAD)  # x0, and SPREAD * x0 where every row of A carries weight (at x0 the softmax of the larger shapes sits on a few rows)


@pytest.mark.parametrize("m,n", NC.HESS_SHAPES)
def test_hessian_kernel_against_extended_precision(qn, m, n):
    """|H_dev - H_true|_ij <= B S_ij at x0 and at SPREAD * x0; (1024, 1024) is the shape with several tiles and a long K loop."""
    for scale in SCALES:
        truth, bound, s = NC.truth_at(m, n, scale)
        _check_inside_bound(_device_hessians(qn, m, n, scale)[0], truth, bound, s, f"({m}, {n}) at {scale} x0")


@pytest.mark.parametrize("m,n", NC.HESS_SHAPES)
def test_hessian_structure(qn, m, n):
    """H == H' bit for bit, two calls give identical bits."""
    for scale in SCALES:
        h1, h2 = _device_hessians(qn, m, n, scale)
        assert h1.shape == (n, n)
        assert np.array_equal(h1, h1.T)
        assert np.array_equal(h1, h2)


def test_quadratic_hessian_is_q(qn, qo):
    """obj.hessian(x) of a quadratic equals Q exactly: a symmetric Q, one that is not (rows and columns must not be swapped on the way out), and
    the matrix Quadratic.synthetic generates on the device (compared with the rows the objective itself hands out)."""
    import problems as P
    for n in (5, 77):
        q, b, x0, diag = P.synth_problem(qo, n, 100.0)
        assert np.array_equal(q, q.T)
        skew = q.copy()
        skew[0, n - 1] += 0.25
        for mat in (q, skew):
            obj = qn.Quadratic(mat, b)
            assert np.array_equal(obj.hessian(x0), mat)
            obj.close()
        obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
        h = obj.hessian(x0)
        assert np.array_equal(h, obj.rows(0, n)) and np.array_equal(h, q)
        obj.close()


def test_hessian_rejects_a_point_of_the_wrong_length(qn):
    a, c, mu, x0 = NC.problem(3, 5)
    obj = qn.LogSumExp(a, c, mu)
    with pytest.raises(qn.ErrorInputParams):
        obj.hessian(x0[:-1])
    obj.close()


def test_saturated_softmax(qn):
    """Saturated softmax: one entry of c 800 above the rest: every entry finite, H within the bound of the truth (mu I to 1e-300)."""
    m, n = 96, 64
    a, c, mu, x0 = NC.problem(m, n)
    c = c.copy()
    c[17] += 800.0
    obj = qn.LogSumExp(a, c, mu)
    h = obj.hessian(x0)
    obj.close()
    truth, bound, s = NC.hessian_truth_and_bound(a, c, mu, x0)
    _check_inside_bound(h, truth, bound, s, "saturated (96, 64)")
    assert np.array_equal(h, h.T)


_host_runs = {}


def _gpu_run(qn, m, n, lsname, memoize, lu, device):
    a, c, mu, x0 = NC.problem(m, n)
    s = qn.Newton(NC.TOL, x0)
    s.memoize = memoize
    if lu:
        s.set_option("newton_pivoted_lu", 1)
    s.set_trace(NC.MAX_ITER)
    if device:
        obj = qn.LogSumExp(a, c, mu)
        s.minimize(NC.ls_of(qn, lsname), obj, NC.MAX_ITER, NC.MAX_LS)
        conv = s.has_converged(obj(s.x()))
        obj.close()
    else:
        fn = PC.lse_hess_fn(a, c, mu)

        def oracle(x):
            f, g, h = fn(x)
            return qn.FuncEvalMultivariate(f, g).with_hessian(h)
        s.minimize(NC.ls_of(qn, lsname), oracle, NC.MAX_ITER, NC.MAX_LS)
        conv = s.has_converged(oracle(s.x()))
    tr = s.trace()[0]
    out = (s.k(), tr[0]["t"], conv, s.x())
    s.close()
    return out


def _host_run(qn, m, n, lsname, memoize, lu):
    key = (m, n, lsname, memoize, lu)
    if key not in _host_runs:
        _host_runs[key] = _gpu_run(qn, m, n, lsname, memoize, lu, device=False)
    return _host_runs[key]


def _compare_runs(qn, qo, m, n, lsname, memoize, lu):
    st, k_ref, t_ref, x_ref = NC.oracle_run(qo, m, n, lsname)
    assert st == qo.OK
    k_h, t_h, conv_h, x_h = _host_run(qn, m, n, lsname, memoize, lu)
    k_d, t_d, conv_d, x_d = _gpu_run(qn, m, n, lsname, memoize, lu, device=True)
    dist_h, dist_d = float(np.linalg.norm(x_h - x_ref)), float(np.linalg.norm(x_d - x_ref))
    floor = NC.x_floor(n, x_ref)
    print(f"({m}, {n}) {lsname} memoize={memoize} lu={lu}: k oracle/host/device = {k_ref}/{k_h}/{k_d}  t0 = {t_ref!r}/{t_h!r}/{t_d!r}  "
          f"host-closure distance {dist_h:.3e}  device distance {dist_d:.3e}  floor {floor:.3e}")
    assert k_d == k_h == k_ref
    if t_ref != t_h or t_ref != t_d:
        print(f"    t0 in units of the last place of the oracle's: host {(t_h - t_ref) / np.spacing(t_ref):+.0f}, device {(t_d - t_ref) / np.spacing(t_ref):+.0f}")
    assert _t_equal(t_h, t_ref, lsname, "host") and _t_equal(t_d, t_ref, lsname, "device")
    assert conv_d and conv_h
    assert dist_d <= max(8.0 * HOST_DIST[(m, n, lsname, memoize, lu)], floor)


@pytest.mark.parametrize("memoize", [0, 1])
@pytest.mark.parametrize("lsname", ["mt", "bt"])
@pytest.mark.parametrize("m,n", NC.RUN_SHAPES)
def test_newton_on_device_logsumexp(qn, qo, m, n, lsname, memoize):
    """Whole runs through the blocked Cholesky: the factorisation and Newton's state machine over the 10-12 iterations these problems take."""
    _compare_runs(qn, qo, m, n, lsname, memoize, 0)


@pytest.mark.parametrize("lsname", ["mt", "bt"])
def test_newton_on_device_logsumexp_pivoted_lu(qn, qo, lsname):
    """The pivoted LU reads the whole matrix -- the mirrored upper triangle."""
    _compare_runs(qn, qo, *NC.LU_SHAPE, lsname, 1, 1)


def test_two_rank_context_is_rejected(qn):
    """Newton on log-sum-exp, and Objective.hessian, are single-GPU: a row-sharded context answers ErrorInputParams."""
    from thread_ranks import run_ranks
    a, c, mu, x0 = NC.problem(96, 64)

    def body(rank, world, group):
        ctx = qn.Context(0, rank=rank, world=world, host_allgather=group.allgather_fn(rank))
        obj = qn.LogSumExp(a, c, mu, ctx=ctx)
        s = qn.Newton(NC.TOL, x0, ctx=ctx)
        with pytest.raises(qn.ErrorInputParams):
            s.minimize(qn.MoreThuente(), obj, NC.MAX_ITER, NC.MAX_LS)
        with pytest.raises(qn.ErrorInputParams):
            obj.hessian(x0)
        s.close()
        obj.close()
        ctx.close()
        return True
    assert run_ranks(2, body, timeout=60.0) == [True, True]


def test_newton_example_cpp():
    """examples/newton_example.cpp: Newton through the C++ mirror (include/qn_solver.hpp) -- the reference's newton_morethuente problem as a
    closure carrying its Hessian, then a device LogSumExp beside the same problem as a host closure."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "newton_example.bin")
    assert os.path.exists(exe), "examples/newton_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("newton example ok")
