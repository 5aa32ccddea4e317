"""The problems the nonlinear-CG tests share (tests/test_ref_cg.py licenses the windows, tests/test_gpu_cg.py uses them): lbfgs_cases' problems --
the separable quartic ("host": a host closure), the log-sum-exp problem ("lse") and the synthetic quadratic with kappa = 1e2 ("quad": the device
objective) -- at n = 7 (odd, padding) and 2050 (two workgroups, the last one ragged), StrongWolfe(1e-4, 0.1) and BackTracking(1e-4, 0.5), every
variant, tol 1e-10, at most 30 iterations.  Every restatement run is made once and kept.

THE LICENCE of a window (the method of tests/test_ref_lbfgs.py): the case runs with numpy.dot, with math.fsum of the products and with every dot
product summed in reversed order; the window ends at the first iteration where the iterates differ by more than 1e-11 max(1, ||x||) (or the
step t by more than 1e-11 |t|, or beta by more than 1e-11 max(1, |beta|): the GPU tests compare t and the last beta too), n_evals differs, the restart pattern (beta == 0) differs, or lbfgs_cases.above_f_floor's rule fails.  The GPU sums in a fourth order and is compared
inside the window at 1e-9 max(1, ||x||).

A DEVICE OBJECTIVE ("lse", "quad", SparseQuadratic, the device closure) is also ANOTHER EVALUATION of the function: its f and g differ from the host
function's by a few ulp (other exp / log, FMA accumulations, other summation orders), which no dot-product order of the restatement models.  Under an
interpolating search that matters long before above_f_floor's 1e4 ulp: the cubic step is made of f's DIFFERENCES, so an error of u ulp of f moves t by
about u eps |f| / (f_k - f_{k+1}).  So those cases run twice more, with every evaluation moved pseudo-randomly (seeded by the point) by up to 8 ulp of f
and 2 ulp of each g_i -- at least four times what the device objectives' own roundings come to (exp and log within 2 ulp, sums of 96 to 2050 terms in
blocks) -- and the window ends where such a run differs from the plain one by more than 2.5e-10 in x, t or beta (a quarter of the GPU tests' 1e-9), or in
any decision.  The log-sum-exp problem of lbfgs_cases at n = 7 converges in 13-16 iterations and gives 5 iterations under that rule with StrongWolfe;
as "another case, not a shorter window", n = 7 uses the same generator with mu = 0.01 and 3 x0 (27-30 iterations to converge).

NOT in the set: the quadratic at n = 7 under StrongWolfe -- the interpolated step lands on the exact line minimiser and the sign of phi' there is
decided by the summation order -- and any n = 2 run (they converge inside 5-11 iterations)."""
import functools
import zlib

import numpy as np

import lbfgs_cases as L
import ref_cg as RC
import ref_spg as R
import ref_wolfe as W
import spg_cases as S

WINDOW = 30
MIN_WINDOW = 8
TOL = 1e-10
LICENCE = 1e-11
SIZES = (7, 2050)
SEARCHES = ("wolfe", "bt")
ORACLES = ("host", "lse", "quad")
WOLFE = (1e-4, 0.1)
CASES = [(v, o, ls, n) for v in RC.VARIANTS for o in ORACLES for ls in SEARCHES for n in SIZES if not (o == "quad" and n == 7 and ls == "wolfe")]
SHAPE_SIZES = (2, 7, 4099, (1 << 21) + 3)  # 4099: three workgroups, a ragged last one; 2^21 + 3: the grid-stride loop wraps


def rev_dot(a, b):
    return float(np.dot(a[::-1], b[::-1]))


DOTS = {"numpy": np.dot, "fsum": R.fsum_dot, "reversed": rev_dot}


ROUNDING_LICENCE = 2.5e-10
LSE7_MU, LSE7_X0_SCALE = 0.01, 3.0


@functools.lru_cache(maxsize=None)
def lse_problem(n):
    """(a, c, mu, x0): lbfgs_cases' problem; at n = 7 its generator with a weaker regulariser and a start three times as far out (see above)"""
    a, c, mu, x0, _, _ = L.lse_problem(n)
    return (a, c, LSE7_MU, LSE7_X0_SCALE * x0) if n == 7 else (a, c, mu, x0)


def oracle_fn(oracle, n):
    if oracle == "host":
        return L.separable_problem(n)
    if oracle == "lse":
        a, c, mu, x0 = lse_problem(n)
        return S.lse_fn(a, c, mu), x0
    return L.oracle_fn(oracle, n)


def rounded_otherwise(fn, seed, ulp_f=8.0, ulp_g=2.0):
    """the same function as another evaluation of it: f moved by up to ulp_f ulp, every g_i by up to ulp_g ulp, seeded by the point"""
    def moved(x):
        f, g = fn(x)
        rng = np.random.default_rng(zlib.crc32(np.ascontiguousarray(x).tobytes()) ^ seed)
        return float(f + ulp_f * rng.uniform(-1.0, 1.0) * np.spacing(abs(f))), g + ulp_g * rng.uniform(-1.0, 1.0, g.size) * np.spacing(np.abs(g))
    return moved


def line_search(kind, dot=np.dot):
    if kind == "wolfe":
        return W.StrongWolfe(WOLFE[0], WOLFE[1], dot=dot)
    return R.BackTracking(1e-4, 0.5, dot=dot)


def run_ref(fn, x0, variant, ls, iters, powell_nu=0.2, restart_every=0, dot=np.dot, max_ls=50, tol=TOL, solver=None):
    """The restatement on one case: (solver object, oracle, status).  `solver`: continue that one (a warm restart)."""
    o = R.CountingOracle(fn)
    s = solver or RC.NonlinearCG(tol, x0, variant=variant, powell_nu=powell_nu, restart_every=restart_every, dot=dot)
    status = "ok"
    try:
        s.minimize(line_search(ls, dot), o, iters, max_ls)
    except R.MaxIterReached:
        status = "max_iter"
    except W.NotDescent:
        status = "not_descent"
    return s, o, status


@functools.lru_cache(maxsize=None)
def ref_case(variant, oracle, ls, n, order="numpy", powell_nu=0.2, restart_every=0):
    fn, x0 = oracle_fn(oracle, n)
    return run_ref(fn, x0, variant, ls, WINDOW, powell_nu=powell_nu, restart_every=restart_every, dot=DOTS[order])


def agreeing(a, others, within=LICENCE):
    """(iterations at the front on which the runs agree, the worst relative difference in x, t and beta inside them)"""
    w, worst = len(a.trace), 0.0
    for o in others:
        w = min(w, len(o.trace))
    for k in range(w):
        here = 0.0
        for o in others:
            same = a.trace[k]["n_evals"] == o.trace[k]["n_evals"] and a.trace[k]["ls_iters"] == o.trace[k]["ls_iters"] and a.updated[k] == o.updated[k]
            dx = float(np.linalg.norm(a.trace_x[k] - o.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k])))
            dt = abs(a.trace[k]["t"] - o.trace[k]["t"]) / abs(a.trace[k]["t"])
            db = abs(a.betas[k] - o.betas[k]) / max(1.0, abs(a.betas[k]))
            if not same or not dx <= within or not dt <= within or not db <= within:
                return k, worst
            here = max(here, dx, dt, db)
        worst = max(worst, here)
    return w, worst


@functools.lru_cache(maxsize=None)
def licence(variant, oracle, ls, n, powell_nu=0.2, restart_every=0):
    """(window, worst disagreement inside it) of one case"""
    a = ref_case(variant, oracle, ls, n, "numpy", powell_nu, restart_every)[0]
    others = [ref_case(variant, oracle, ls, n, order, powell_nu, restart_every)[0] for order in ("fsum", "reversed")]
    w, worst = agreeing(a, others)
    if oracle != "host":
        fn, x0 = oracle_fn(oracle, n)
        w = min(w, rounding_window(a, fn, x0, variant, ls, powell_nu=powell_nu, restart_every=restart_every))
    return min(w, L.above_f_floor(a, ls)), worst


def rounding_window(a, fn, x0, variant, ls, iters=WINDOW, **kw):
    moved = [run_ref(rounded_otherwise(fn, seed), x0, variant, ls, iters, **kw)[0] for seed in (1, 2)]
    return agreeing(a, moved, ROUNDING_LICENCE)[0]


def licence_of(fn, x0, variant, ls, iters=WINDOW, **kw):
    """the same licence for a problem outside CASES: (the numpy.dot run, window, worst disagreement)"""
    runs = [run_ref(fn, x0, variant, ls, iters, dot=d, **kw)[0] for d in DOTS.values()]
    w, worst = agreeing(runs[0], runs[1:])
    w = min(w, rounding_window(runs[0], fn, x0, variant, ls, iters, **kw))  # (every user is a device objective)
    return runs[0], min(w, L.above_f_floor(runs[0], ls)), worst


def window(variant, oracle, ls, n, powell_nu=0.2, restart_every=0):
    return licence(variant, oracle, ls, n, powell_nu, restart_every)[0]


# the cases of the restart rules (windows licensed like every other): restart_every = 3, and Powell's test on and off
EVERY = ("pr+", "host", "wolfe", 2050, float("inf"), 3)  # (Powell's test off: an unscheduled restart would restart the count)
POWELL = ("fr", "lse", "bt", 2050)


# ---- the shape test: beta of the second iteration against longdouble sums of the same vectors ----
EPS = float(np.finfo(np.float64).eps)


def ld_sums(g, gp, d):
    """the seven sums of the formulas in longdouble, and sum |a_i b_i| of each, on y = fl(g+ - g) as the kernel forms it"""
    y = gp - g
    ld = np.longdouble
    pairs = dict(gpgp=(gp, gp), gpy=(gp, y), dy=(d, y), gpd=(gp, d), yy=(y, y), dd=(d, d), gg=(g, g))
    exact = {k: float(np.sum(a.astype(ld) * b.astype(ld))) for k, (a, b) in pairs.items()}
    mags = {k: float(np.sum(np.abs(a.astype(ld) * b.astype(ld)))) for k, (a, b) in pairs.items()}
    return exact, mags


USES = {"fr": ("gpgp", "gg"), "pr+": ("gpy", "gg"), "hs+": ("gpy", "dy"), "dy": ("gpgp", "dy"), "hz": ("gpy", "yy", "gpd", "dy", "dd", "gg")}


def beta_bound(variant, n, exact, mags):
    """(beta from the exact sums, the bound on |beta_gpu - beta|): every float64 sum of n products, in ANY order, lies within n eps sum |a_i b_i| of
    the exact one (Higham, Accuracy and Stability, (3.5), first order: gamma_n ~ n eps; one more eps for the accumulator's last rounding is inside
    the n + 1 used here).  Each sum the variant uses is moved to both ends of that interval and the formula evaluated at every corner -- it is
    monotone in each sum on intervals that do not contain a zero of a denominator, which is asserted -- and the formula's own operations (at most
    9 roundings, each relative eps on an intermediate no larger than the largest corner value in magnitude, and HZ's two terms) add 16 eps of the
    largest magnitude met."""
    names = USES[variant]
    e = {k: (n + 1) * EPS * mags[k] for k in names}
    for k in ("gg", "dy"):
        if k in names:
            assert abs(exact[k]) > 4.0 * e[k], (k, exact[k], e[k])  # the denominator's interval keeps clear of zero
    centre = RC.beta_formula(variant, **exact)
    worst, big = 0.0, abs(centre)
    for corner in range(1 << len(names)):
        v = dict(exact)
        for i, k in enumerate(names):
            v[k] = exact[k] + (e[k] if corner >> i & 1 else -e[k])
        for k in ("yy", "dd", "gg", "gpgp"):
            v[k] = max(v[k], 0.0)
        b = RC.beta_formula(variant, **v)
        worst, big = max(worst, abs(b - centre)), max(big, abs(b))
        if variant == "hz":
            big = max(big, abs(v["gpy"] / v["dy"]), abs(2.0 * v["yy"] * v["gpd"] / (v["dy"] * v["dy"])))
    return centre, worst + 16.0 * EPS * big
