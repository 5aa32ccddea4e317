"""GPU tests of the steady iteration's machine steps as straight-line code (csrc/qn_sym2.hip.h qn_s2_fast_step, set_option("machine_fast_steps", v)):
the accept-reduce's prologue takes evaluation -> Wolfe test -> accepted -> request for the vectors, the update tiles' prologue takes the five sums ->
qn_st_after_next -> request for the pass, each by calling the generic machine's own state functions one after the other; whatever they leave running
(a trial that is not accepted, a step below tol, the end of an iteration whose iterate is traced) goes on in the generic machine.  Nothing may be decided
differently: with the option 1 against 0 the trace records, every iterate and the inverse Hessian are equal bit for bit, and so are the launches, the
oracle evaluations, the passes over H and the status.  qn_stats.fast_machine_steps says that the steps ran.

Shapes: n = 1024 (n == n_pad >= 8 * 128: the evaluation kernel's general body, s2_vec_kernel<false> / s2_hreduce_kernel<false>) and n = 4096 (the
instantiations with 32 touch workgroups behind the two-items-and-a-sliver evaluation, as mover + multiplier waves and as round 5's kernel)."""
import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

_objs = {}


def _problem(qn, n):
    """the synthetic quadratic of size n, built once per session"""
    if n not in _objs:
        diag = P.synth_diag(n)
        b, x0 = P.synth_vectors(n)
        _objs[n] = (qn.Quadratic.synthetic(n, P.SEED, diag, b), x0)
    return _objs[n]


def _ls(qn, lsname):
    return qn.MoreThuente() if lsname == "mt" else qn.BackTracking(1e-4, 0.5)


def _run(qn, method, lsname, obj, x0, iters, fast, sync=0, opts=(), tol=1e-10):
    s = (qn.BFGS if method == "bfgs" else qn.DFP)(tol, x0)
    s.set_trace(iters, with_x=True)
    s.configure("machine_fast_steps", fast)
    for name, v in opts:
        s.configure(name, v)
    s.set_sync_mode(sync)
    st = 0
    try:
        s.minimize(_ls(qn, lsname), obj, iters, 20)
    except qn.MaxIterReached:
        st = 1
    return s, st


def _same_run(a, st_a, b, st_b):
    (tr_a, xs_a), (tr_b, xs_b) = a.trace(), b.trace()
    assert st_a == st_b and tr_a == tr_b
    assert np.array_equal(xs_a, xs_b) and np.array_equal(a.x(), b.x())
    assert np.array_equal(a.approx_inv_hessian(), b.approx_inv_hessian())
    sa, sb = a.stats(), b.stats()
    for k in ("launches", "oracle_evals", "h_passes", "iterations"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])


CASES = [(1024, ()), (4096, ()), (4096, (("eval_mover_multiplier", 0),))]  # general body; touch instantiations behind the ring; ... behind the pair instance


@pytest.mark.parametrize("n,opts", CASES, ids=["1024", "4096-ring", "4096-pair"])
@pytest.mark.parametrize("method", ["bfgs", "dfp"])
@pytest.mark.parametrize("sync", [0, 1], ids=["pipelined", "sync"])
def test_more_thuente_steps_change_no_bit_and_are_taken(qn, n, opts, method, sync):
    """12 iterations of More-Thuente.  Every steady iteration takes one step per prologue: at least 2 (iterations - 1) in all (the first iteration
    of a cold call may take the generic path); none with the option off.  (Synchronous mode: the one-workgroup launch that runs the machine between
    the service launches holds both steps.)"""
    obj, x0 = _problem(qn, n)
    iters = 12
    off, st0 = _run(qn, method, "mt", obj, x0, iters, 0, sync, opts)
    on, st1 = _run(qn, method, "mt", obj, x0, iters, 1, sync, opts)
    assert off.stats()["path"] & 16 and on.stats()["path"] & 16  # QN_PATH_SYM2
    assert len(on.trace()[0]) == iters
    _same_run(on, st1, off, st0)
    f0, f1 = off.stats()["fast_machine_steps"], on.stats()["fast_machine_steps"]
    print("fast_machine_steps off / on:", f0, f1, "iterations:", on.stats()["iterations"])
    assert f0 == 0
    assert f1 >= 2 * (iters - 1)


@pytest.mark.parametrize("n,opts", CASES, ids=["1024", "4096-ring", "4096-pair"])
def test_backtracking_takes_the_generic_path_in_the_accept_reduce(qn, n, opts):
    """BackTracking(1e-4, 0.5): the accept-reduce consumes an evaluation behind QN_ST_BT_AFTER -- not the straight-line step's case -- so only the
    update tiles' prologue takes its step: at most one per iteration (one request for the vectors per iteration), where More-Thuente takes two."""
    obj, x0 = _problem(qn, n)
    iters = 12
    off, st0 = _run(qn, "bfgs", "bt", obj, x0, iters, 0, 0, opts)
    on, st1 = _run(qn, "bfgs", "bt", obj, x0, iters, 1, 0, opts)
    _same_run(on, st1, off, st0)
    f0, f1 = off.stats()["fast_machine_steps"], on.stats()["fast_machine_steps"]
    print("fast_machine_steps off / on:", f0, f1)
    assert f0 == 0
    assert iters - 1 <= f1 <= iters  # the update tiles' share alone: the accept-reduce's is 0


@pytest.mark.parametrize("n", [1024, 4096])
def test_converged_run_and_continued_call(qn, n):
    """tol = 1e-3 run to convergence (qn_st_after_next leaves QN_ST_ITER_END: the generic machine ends the run), then set_x(x + 0.25) and 15 more
    iterations on the inverse Hessian the first call left."""
    obj, x0 = _problem(qn, n)
    outs = []
    for fast in (0, 1):
        s = qn.BFGS(1e-3, x0)
        s.set_trace(200, with_x=True)
        s.configure("machine_fast_steps", fast)
        ls = qn.MoreThuente()
        st1 = 0
        try:
            s.minimize(ls, obj, 200, 20)
        except qn.MaxIterReached:
            st1 = 1
        k1, x1, tr1, stats1 = s.k(), s.x(), s.trace(), s.stats()
        s.set_x(x1 + 0.25)
        st2 = 0
        try:
            s.minimize(ls, obj, 15, 20)
        except qn.MaxIterReached:
            st2 = 1
        outs.append((st1, k1, x1, tr1, stats1, st2, s.k(), s.x(), s.trace(), s.stats(), s.approx_inv_hessian()))
    a, b = outs
    assert a[0] == b[0] == 0  # converged
    assert a[1] == b[1] and np.array_equal(a[2], b[2])
    assert a[3][0] == b[3][0] and np.array_equal(a[3][1], b[3][1])
    assert a[5] == b[5] and a[6] == b[6] and np.array_equal(a[7], b[7])
    assert a[8][0] == b[8][0] and np.array_equal(a[8][1], b[8][1])
    assert np.array_equal(a[10], b[10])
    for i in (4, 9):
        for k in ("launches", "oracle_evals", "h_passes", "iterations"):
            assert a[i][k] == b[i][k], (i, k)
    assert a[4]["fast_machine_steps"] == 0 and a[9]["fast_machine_steps"] == 0
    assert b[4]["fast_machine_steps"] > 0


@pytest.mark.parametrize("n", [1024, 4096])
def test_warm_continuation(qn, n):
    """Two calls of 5 iterations: the second continues warm (no evaluation at x, the direction pending in its lazy form)."""
    obj, x0 = _problem(qn, n)
    outs = []
    for fast in (0, 1):
        s = qn.BFGS(1e-10, x0)
        s.set_trace(5, with_x=True)
        s.configure("machine_fast_steps", fast)
        ls = qn.MoreThuente()
        legs = []
        for leg in range(2):
            st = 0
            try:
                s.minimize(ls, obj, 5, 20)
            except qn.MaxIterReached:
                st = 1
            legs.append((st, s.trace(), s.x(), s.stats()))
        outs.append((legs, s.approx_inv_hessian()))
    (la, ha), (lb, hb) = outs
    assert np.array_equal(ha, hb)
    for x, y in zip(la, lb):
        assert x[0] == y[0] and x[1][0] == y[1][0] and np.array_equal(x[1][1], y[1][1]) and np.array_equal(x[2], y[2])
        for k in ("launches", "oracle_evals", "h_passes", "iterations"):
            assert x[3][k] == y[3][k], k
        assert x[3]["fast_machine_steps"] == 0
    assert lb[0][3]["fast_machine_steps"] >= 2 * 4 and lb[1][3]["fast_machine_steps"] >= 2 * 4  # (per call)


def test_bounded_machine_is_untouched(qn):
    """BFGSB + MoreThuenteB at n = 1024: the bounded runs' prologues hold no straight-line step; the option changes nothing and counts nothing."""
    n = 1024
    obj, x0 = _problem(qn, n)
    lb, ub = x0 - 0.3, x0 + 0.3
    outs = []
    for fast in (0, 1):
        s = qn.BFGSB.new(1e-9, x0, lb, ub)
        s.set_trace(12, with_x=True)
        s.configure("machine_fast_steps", fast)
        ls = qn.MoreThuenteB.new(n).with_lower_bound(lb).with_upper_bound(ub)
        st = 0
        try:
            s.minimize(ls, obj, 12, 30)
        except qn.MaxIterReached:
            st = 1
        outs.append((st, s.trace(), s.x(), s.stats(), ls.t_max()))
    a, b = outs
    assert a[3]["path"] & 16
    assert a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and np.array_equal(a[2], b[2]) and a[4] == b[4]
    for k in ("launches", "oracle_evals", "h_passes", "iterations"):
        assert a[3][k] == b[3][k], k
    assert a[3]["fast_machine_steps"] == 0 and b[3]["fast_machine_steps"] == 0
