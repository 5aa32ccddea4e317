"""SpectralProjectedNewton + GLLQuadratic on Quadratic.synthetic beside the Newton iteration on the same matrix, in one process
(tools/newton_time.py's protocol): wall time of `minimize` between two context synchronisations, per iteration.
  (a) the Cholesky factor made in every iteration (QN_OPT_PNEWTON_REUSE_FACTOR 0)
  (b) the factor kept (default): the steady-state iteration is the solve, the evaluation and the vector kernels
  (c) Newton + More-Thuente, five alternating repetitions with (a): its min-max is the run-to-run spread (a) is judged against
usage: bench_pnewton.py [n ...] [--profile-b]   (--profile-b: only a warm (b) run, for a kernel trace)"""
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

qn = ge.load_package()
import problems as P  # noqa: E402

ITERS = 10
args = [a for a in sys.argv[1:] if not a.startswith("--")]
sizes = [int(a) for a in args] or [4096, 8192]
profile_b = "--profile-b" in sys.argv


def timed(make, run):
    s = make()
    qn.default_context().synchronize()
    t0 = time.perf_counter()
    try:
        run(s)
    except qn.MaxIterReached:
        pass
    qn.default_context().synchronize()
    dt = time.perf_counter() - t0
    k = s.k()
    extra = s.newton_factorisations() if hasattr(s, "newton_factorisations") else None
    s.close()
    return dt * 1e3 / max(k, 1), k, extra


for n in sizes:
    diag = P.synth_diag(n)
    b, x0 = P.synth_vectors(n)
    obj = qn.Quadratic.synthetic(n, P.SEED, diag, b)
    lb, ub = np.full(n, -0.05), np.full(n, 0.05)

    def spn(reuse):
        def make():
            s = qn.SpectralProjectedNewton(1e-12, x0, obj, lb, ub)
            s.set_option("pnewton_reuse_factor", reuse)
            return s
        return make
    run_spn = lambda s: s.minimize(qn.GLLQuadratic(1e-4, 10), obj, ITERS, 20)  # noqa: E731
    run_newton = lambda s: s.minimize(qn.MoreThuente(), obj, ITERS, 20)  # noqa: E731
    if profile_b:
        s = spn(1)()
        for _ in range(3):
            try:
                s.minimize(qn.GLLQuadratic(1e-4, 10), obj, ITERS, 20)
            except qn.MaxIterReached:
                pass
        print(f"n={n} profile-b: k={s.k()} factorisations of the last call={s.newton_factorisations()}")
        continue
    timed(spn(0), run_spn)  # warm-up: allocations, code objects
    timed(lambda: qn.Newton(1e-8, x0), run_newton)
    a, c, bb = [], [], []
    for rep in range(5):
        c.append(timed(lambda: qn.Newton(1e-8, x0), run_newton))
        a.append(timed(spn(0), run_spn))
        bb.append(timed(spn(1), run_spn))
    # (b)'s steady state: the first call pays the one factorisation; a second call on the same solver pays none
    s = spn(1)()
    try:
        run_spn(s)
    except qn.MaxIterReached:
        pass
    steady = timed(lambda: s, run_spn)
    out = dict(n=n, iters=ITERS,
               a_ms_per_iter=[round(v[0], 4) for v in a], a_iterations=a[0][1], a_factorisations=a[0][2],
               b_ms_per_iter=[round(v[0], 4) for v in bb], b_factorisations=bb[0][2],
               b_steady_ms_per_iter=round(steady[0], 4), b_steady_factorisations=steady[2],
               c_ms_per_iter=[round(v[0], 4) for v in c], c_iterations=c[0][1])
    out["a_median"] = float(np.median(out["a_ms_per_iter"]))
    out["c_min_max"] = [min(out["c_ms_per_iter"]), max(out["c_ms_per_iter"])]
    out["a_not_slower_than_c"] = out["a_median"] <= out["c_min_max"][1]
    print(json.dumps(out))
