"""The problems the L-BFGS tests share (tests/test_ref_lbfgs.py licenses the windows, tests/test_gpu_lbfgs.py uses them).  Sizes from the
vector kernels' grid (G = ceil(n_pad / 2048), at most 1024): n = 2 (the reference's test size), 7 (odd, padding, m > n), 2050 (two workgroups,
the last one ragged), 2^21 + 2 (the grid-stride loop wraps; m = 3, a separable function).  kappa = 1e2, tol 1e-10, at most 30 iterations, as
pnewton_cases.  Every restatement run is made once and kept.  At the end: REPLAY_CASES, the runs tests/lbfgs_replay.py replays direction by
direction (m up to 32 with the ring wrapping twice, m = 5 at n = 2^21 + 2)."""
import functools

import numpy as np

import problems as P
import ref_lbfgs as RL
import ref_spg as R
import spg_cases as S

WINDOW = 30
TOL = 1e-10
SIZES = (2, 7, 2050)
MEMORIES = (1, 5, 32)
SEARCHES = ("gll", "bt")
ORACLES = ("host", "quad", "lse")
CASES = [(o, ls, m, n) for o in ORACLES for ls in SEARCHES for m in MEMORIES for n in SIZES]
BOX_CASES = [(ls, n, 5) for ls in ("gll", "bt", "btb") for n in (7, 2050)] + [("bt", 2050, 1), ("btb", 2050, 2)]  # (m = 1, 2: the ring wraps inside the short BackTracking windows)
BOX = 0.05
BIG_N, BIG_M, BIG_WINDOW = (1 << 21) + 2, 3, 5
UNIT_N, UNIT_M, UNIT_WINDOW = 64, 16, 12


@functools.lru_cache(maxsize=None)
def quad_problem(n):
    from oracle import qn_oracle as qo
    return S.problem(qo, n)


@functools.lru_cache(maxsize=None)
def lse_problem(n):
    return S.lse_problem(m=96, n=n, seed=3)


def oracle_fn(oracle, n):
    """(fn, x0) of one oracle kind at size n: "host" and "quad" are the synthetic quadratic, "lse" the log-sum-exp problem"""
    if oracle == "lse":
        a, c, mu, x0, _, _ = lse_problem(n)
        return S.lse_fn(a, c, mu), x0
    q, b, x0, _ = quad_problem(n)
    return R.quadratic_fn(q, b), x0


def separable_problem(n=BIG_N):
    """f = sum_i (a_i/2 x_i^2 + 1/4 x_i^4), a_i in [1, 100] on a fixed pattern: cheap at any n"""
    i = np.arange(n, dtype=np.float64)
    a = 1.0 + 99.0 * ((i * 0.6180339887498949) % 1.0)
    x0 = 0.5 + ((i * 0.3819660112501051) % 1.0)

    def fn(x):
        x2 = x * x
        return float(np.sum(0.5 * a * x2 + 0.25 * x2 * x2)), a * x + x2 * x
    return fn, x0


def line_search(kind, lb, ub, dot=np.dot):
    if kind == "gll":
        return R.GLLQuadratic(1e-4, 10, dot=dot)
    if kind == "bt":
        return R.BackTracking(1e-4, 0.5, dot=dot)
    return R.BackTrackingB(1e-4, 0.5, lb, ub, dot=dot)


def run_ref(fn, x0, lb, ub, ls, m, iters, unit=False, dot=np.dot, direction="two_loop", max_ls=50, tol=TOL):
    """The restatement on one case: (solver object, oracle, status).  `stored` on the solver: pairs in the memory after every iteration."""
    o = R.CountingOracle(fn)
    s = RL.LBFGS(tol, x0, lb, ub, m=m, unit_scaling=unit, dot=dot, direction=direction)
    s.stored = []
    status = "ok"
    try:
        s.minimize(line_search(ls, lb, ub, dot), o, iters, max_ls, callback=lambda r: r.stored.append(r.stored_pairs()))
    except R.MaxIterReached:
        status = "max_iter"
    return s, o, status


def free_box(n):
    return np.full(n, -np.inf), np.full(n, np.inf)


@functools.lru_cache(maxsize=None)
def ref_case(oracle, ls, m, n):
    fn, x0 = oracle_fn(oracle, n)
    lb, ub = free_box(n)
    return run_ref(fn, x0, lb, ub, ls, m, WINDOW)


@functools.lru_cache(maxsize=None)
def ref_box_case(ls, n, m=5):
    fn, x0 = oracle_fn("quad", n)
    lb, ub = S.bounds(n, BOX)
    return run_ref(fn, x0, lb, ub, ls, m, WINDOW)


@functools.lru_cache(maxsize=None)
def ref_big():
    fn, x0 = separable_problem()
    lb, ub = free_box(BIG_N)
    return run_ref(fn, x0, lb, ub, "bt", BIG_M, BIG_WINDOW)


# Windows shorter than the leading run of committed pairs: where tests/test_ref_lbfgs.py's self-check found the formulations more than 1e-11
# apart behind this iteration (m = 1 on kappa = 1e2 amplifies a rounding difference fastest)
SHORTER = {("host", "gll", 1, 2): 24, ("quad", "gll", 1, 2): 24, ("lse", "gll", 1, 2050): 26, ("lse", "bt", 32, 2050): 27}
# (BackTracking / BackTrackingB in the box: behind iteration 5 the projected quasi-Newton direction stops descending and the searches run to
# their cap; GLLQuadratic at n = 7: the interpolated step of iteration 21 differs by 6e-10 between the formulations)
BOX_WINDOWS = {("gll", 7): 20, ("gll", 2050): WINDOW, ("bt", 7): 5, ("bt", 2050): 5, ("btb", 7): 5, ("btb", 2050): 5}


def leading_commits(s):
    """iterations up to the first pair that was not committed: behind it these runs have stalled at rounding level (s.y <= eps y.y), where
    every decision is knife-edge"""
    n = 0
    for u in s.updated:
        if not u:
            break
        n += 1
    return n


F_FLOOR = 1e4 * 2.220446049250313e-16


def above_f_floor(s, ls):
    """iterations up to the first whose decrease f_k - f_{k+1} (GLLQuadratic: f_max of its last 10 values - f_{k+1}) is below 1e4 ulp of f: from there the line searches' sufficient-decrease tests
    compare differences that the oracle's own rounding decides (a device objective sums f in another order than the host closure: four
    decimal digits of f's 16 are kept clear of that)"""
    f = [r["f"] for r in s.trace]
    for k in range(len(f) - 1):
        top = max(f[max(0, k - 9):k + 1]) if ls == "gll" else f[k]
        if not top - f[k + 1] >= F_FLOOR * max(1.0, abs(f[k])):
            return k
    return max(0, len(f) - 1)


def window(oracle, ls, m, n):
    s, _, _ = ref_case(oracle, ls, m, n)
    return max(1, min(leading_commits(s), above_f_floor(s, ls), SHORTER.get((oracle, ls, m, n), WINDOW)))


def box_window(ls, n, m=5):
    s, _, _ = ref_box_case(ls, n, m)
    return max(1, min(above_f_floor(s, ls), BOX_WINDOWS[(ls, n)]))


def unit_problem():
    q, b, x0, _ = quad_problem(UNIT_N)
    return R.quadratic_fn(q, b), x0


# ---- a pair rejected while the memory holds pairs (the reason for the ring's spare slot) ----
REJECT_LO, REJECT_HI = 1.0, 4.5
REJECT_X0 = (8.5, 9.0, 9.5)
REJECT_MEMORIES = (1, 2, 5)  # m = 1: the memory is FULL when the pair is rejected; 2, 5: it holds one pair of m
REJECT_WINDOW = 9


def reject_fn(x):
    """f = sum_i h(x_i), convex and C1, h'(u) = u for |u| <= 1, sign(u) for 1 <= |u| <= 4.5, sign(u) (|u| - 3.5) beyond: curved at the start and near the
    minimum, LINEAR between.  From REJECT_X0 the first step lands every coordinate in the linear band (a pair is stored), the next steps stay
    inside it (y = 0 exactly: rejected with pairs in the memory), then the iterate enters the inner curved region and pairs are stored again."""
    a = np.abs(x)
    sg = np.sign(x)
    inner, outer = a <= REJECT_LO, a >= REJECT_HI
    g = np.where(inner, x, np.where(outer, sg * (a - (REJECT_HI - 1.0)), sg))
    h = np.where(inner, 0.5 * a * a, np.where(outer, 0.5 * (a - REJECT_HI) ** 2 + (a - REJECT_HI) + (REJECT_HI - 0.5), a - 0.5))
    return float(np.sum(h)), g


@functools.lru_cache(maxsize=None)
def ref_reject(m, ls="bt"):
    lb, ub = free_box(len(REJECT_X0))
    return run_ref(reject_fn, np.array(REJECT_X0), lb, ub, ls, m, REJECT_WINDOW)


def reject_window(m):
    s, _, _ = ref_reject(m)
    return max(1, min(len(s.trace), above_f_floor(s, "bt")))


def concave_mixed_fn(x):
    """f = -1/2 x_0^2 + 2 x_1^2: the first step is dominated by the convex coordinate (its pair is stored), the later ones run along the concave
    one (s.y < 0: rejected with a pair in the memory)"""
    return float(-0.5 * x[0] ** 2 + 2.0 * x[1] ** 2), np.array([-x[0], 4.0 * x[1]])


CONCAVE_X0, CONCAVE_WINDOW = (0.1, 1.0), 5


# ---- the replay's cases (tests/lbfgs_replay.py; licensed by tests/test_ref_lbfgs_replay.py, run on the GPU by tests/test_gpu_lbfgs_replay.py) ----
def _replay_case(name, prob, n, m, ls, iters, **kw):
    """prob: "quad" / "lse" / "sep" (the problems above), "reject", "concave", "zero" (f = x.x / 2 from (3, 4): g = 0 exactly after one step).
    box: S.bounds(n, BOX); calls: minimize calls of `iters` iterations each, replayed as one run; wraps: the case exists to wrap the ring
    (2 (m + 1) committed pairs at least; 66 at m = 32); cpu_n: the size the float64 stand-in runs at where n is too large for it."""
    c = dict(name=name, prob=prob, n=n, m=m, ls=ls, iters=iters, box=False, memoize=None, unit=False, tol=TOL, calls=1, wraps=False, cpu_n=None)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


REPLAY_SMALL_M = (1, 2, 3, 4, 5, 8)
REPLAY_CASES = (
    # m = 32, full and wrapping: k passes through 1 .. 32 (every count of every Gram group), then the head goes round more than once
    [_replay_case(f"m32-{p}-{ls}-n{n}", p, n, 32, ls, 72, wraps=True) for p, ls, n in (("quad", "bt", 64), ("quad", "gll", 64), ("sep", "bt", 2050), ("sep", "gll", 2050))]
    # small memories: a Gram group exactly full (m = 4, 8), the first element of the next (m = 5), m > n (n = 7, m = 8)
    + [_replay_case(f"wrap-m{m}-n{n}", "sep", n, m, "bt", 2 * (m + 1) + 4, wraps=True) for m in REPLAY_SMALL_M for n in (7, 2050)]
    # the line searches, each with the loop's own evaluations (memoize = 0) and with the search's last trial reused (memoize = 1)
    + [_replay_case(f"{ls}-memo{memo}", "lse", 2050, 5, ls, 25, memoize=memo) for ls in ("bt", "gll", "sw") for memo in (0, 1)]
    # the box: to the iteration cap at n = 2050; at n = 7 for 6 iterations (from the seventh on the projected direction stops descending, both searches
    # run to their cap of 50 halvings and a step of 1e-13 |d| is below what any bound can tell apart: more than a fifth of 30 iterations would prove
    # nothing, and which of them do differs between summation orders)
    + [_replay_case(f"box-{ls}-n{n}", p, n, 5, ls, it, box=True) for ls in ("bt", "btb") for p, n, it in (("quad", 7, 6), ("lse", 2050, WINDOW))]
    # rejected pairs and the reset
    + [_replay_case(f"reject-m{m}", "reject", 3, m, "bt", it) for m, it in zip(REJECT_MEMORIES, (6, 7, 9))]  # (to convergence)
    + [_replay_case("concave-m2", "concave", 2, 2, "bt", CONCAVE_WINDOW), _replay_case("zero-gradient-reset", "zero", 2, 5, "bt", 3, tol=0.0)]
    + [_replay_case("unit-scaling", "quad", UNIT_N, UNIT_M, "bt", 24, unit=True)]
    # the grid-stride loop wraps while two Gram groups run (k = 5: groups of 4 + 1)
    + [_replay_case("grid-wraps-m5", "sep", BIG_N, 5, "bt", 7, cpu_n=4098)]
    # k and head survive the call boundary
    + [_replay_case("warm-restart", "sep", 2050, 5, "gll", 20, calls=2)]
)


def replay_problem(case, n=None):
    """(fn, x0, lb, ub) of a replay case"""
    n = case["n"] if n is None else n
    prob = case["prob"]
    if prob == "sep":
        fn, x0 = separable_problem(n)
    elif prob == "reject":
        fn, x0 = reject_fn, np.array(REJECT_X0)
    elif prob == "concave":
        fn, x0 = concave_mixed_fn, np.array(CONCAVE_X0)
    elif prob == "zero":
        fn, x0 = (lambda x: (0.5 * float(x @ x), x.copy())), np.array([3.0, 4.0])
    else:
        fn, x0 = oracle_fn("lse" if prob == "lse" else "host", n)
    lb, ub = S.bounds(n, BOX) if case["box"] else free_box(n)
    return fn, np.asarray(x0, dtype=np.float64), lb, ub
