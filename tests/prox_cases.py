"""What tests/test_ref_prox.py (CPU) and tests/test_gpu_prox.py (GPU) share: the problems of SpectralProximalGradient's tests, the restatement's
runs (each made once and kept), and the windows.

WINDOW CASES (check 8): (kind, shape) -> the smooth part, x0, the penalty and the box.
    quadratic 64            spg_cases.problem, scalar l1 = 0.5, free
    quadratic 1000          the same, l1 per entry (0.5, every seventh entry unpenalised), box +-0.05
    logistic (96, 64)       logistic_cases.problem, l1 = 2 with the first column unpenalised, lb = 0
    sparse logistic (64, 20000)   sparse_logistic_cases.problem, scalar l1 = 0.25, free
    multinomial (40, 13, 5) multinomial_cases.problem, l1 = 1 with the first feature unpenalised in every class, free
each under GLLQuadratic(1e-4, 10) ("gll") and BackTracking(1e-4, 0.5) ("bt").

THE WINDOW of a case is the largest number of leading iterations, 30 at the most, over which the restatement takes the same decisions (n_evals and
ls_iters of every iteration) with numpy.dot, math.fsum and a reversed-order sum for every sum the solver forms.  WINDOWS states them;
tests/test_ref_prox.py::test_window_self_check computes them again and asserts this table.

WHOLE RUNS (check 9): L1 logistic regression (l1 = 2) and L1 least squares (l1 = 5) as host closures at (96, 64), (40, 65), (257, 200), free and
with lb = 0; one unpenalised column (the first), mu = 1e-3, x0 = 0, GLLQuadratic(1e-4, 10) to 1e-7.
"""
import functools

import numpy as np

import logistic_cases as LC
import multinomial_cases as MC
import ref_logistic as RL
import ref_multinomial as RM
import ref_prox as RP
import ref_spg as R
import sparse_logistic_cases as SLC

MAX_WINDOW = 30
TOL = 1e-10
MAX_LS = 50
SEARCHES = ("gll", "bt")
WINDOW_KINDS = (("quadratic", (64,)), ("quadratic", (1000,)), ("logistic", (96, 64)), ("sparse_logistic", (64, 20000)), ("multinomial", (40, 13, 5)))
WINDOW_CASES = [(kind, shape, ls) for kind, shape in WINDOW_KINDS for ls in SEARCHES]
DOTS = {"numpy": np.dot, "fsum": R.fsum_dot, "reversed": RP.reversed_dot}
# computed by window() on the CPU; asserted by tests/test_ref_prox.py::test_window_self_check
WINDOWS = {case: 30 for case in WINDOW_CASES}
WINDOWS[("sparse_logistic", (64, 20000), "bt")] = 28

RUN_SHAPES = ((96, 64), (40, 65), (257, 200))
RUN_CASES = [(kind, m, n, boxed) for kind in ("logistic", "least_squares") for (m, n) in RUN_SHAPES for boxed in (False, True)]
RUN_L1 = {"logistic": 2.0, "least_squares": 5.0}
RUN_MU = 1e-3
RUN_TOL = 1e-7
RUN_CAP = 500


def line_search(ls):
    return RP.GLLQuadratic(1e-4, 10) if ls == "gll" else RP.BackTracking(1e-4, 0.5)


def l1_of(kind, shape):
    """the penalty of a window case: a scalar or n entries"""
    if kind == "quadratic":
        if shape[0] == 64:
            return 0.5
        v = np.full(shape[0], 0.5)
        v[::7] = 0.0
        return v
    if kind == "logistic":
        v = np.full(shape[1], 2.0)
        v[0] = 0.0
        return v
    if kind == "sparse_logistic":
        return 0.25
    m, n, k = shape
    v = np.full(k * n, 1.0)
    v[::n] = 0.0  # class-major: feature 0 of every class
    return v


def box_of(kind, shape):
    if kind == "quadratic" and shape[0] == 1000:
        return np.full(1000, -0.05), np.full(1000, 0.05)
    if kind == "logistic":
        return np.zeros(shape[1]), np.full(shape[1], np.inf)
    return None, None


def smooth(kind, shape, qo=None):
    """(fn, x0) of a window case's smooth part on the host"""
    if kind == "quadratic":
        import spg_cases as S
        q, b, x0, _ = S.problem(qo, shape[0])
        return R.quadratic_fn(q, b), x0
    if kind == "logistic":
        a, y, w, mu, x0, _ = LC.problem(*shape)
        return RL.logistic_fn(a, y, w, mu), x0
    if kind == "sparse_logistic":
        pr = SLC.problem(*shape)
        return RL.logistic_fn(pr["a"], pr["y"], pr["w"], pr["mu"]), pr["x0"]
    a, y, w, k, mu, x0, _ = MC.problem(*shape)
    return RM.multinomial_fn(a, y, w, k, mu), x0


_runs = {}


def run_ref(kind, shape, ls, qo=None, order="numpy", iters=MAX_WINDOW, faults=()):
    """The restatement on one window case: (solver object, oracle, status); kept"""
    key = (kind, shape, ls, order, iters, tuple(faults))
    if key not in _runs:
        fn, x0 = smooth(kind, shape, qo)
        lb, ub = box_of(kind, shape)
        o = R.CountingOracle(fn)
        s = RP.SpectralProximalGradient(TOL, x0, o, l1_of(kind, shape), lb, ub, dot=DOTS[order], faults=faults)
        status = "ok"
        try:
            s.minimize(line_search(ls), o, iters, MAX_LS)
        except R.MaxIterReached:
            status = "max_iter"
        _runs[key] = (s, o, status)
    return _runs[key]


def same_decisions(a, others):
    """the leading iterations over which every run takes a's decisions"""
    w = min([len(a.trace)] + [len(o.trace) for o in others])
    for k in range(w):
        for o in others:
            if a.trace[k]["n_evals"] != o.trace[k]["n_evals"] or a.trace[k]["ls_iters"] != o.trace[k]["ls_iters"]:
                return k
    return w


def window(kind, shape, ls, qo=None):
    a = run_ref(kind, shape, ls, qo)[0]
    return min(MAX_WINDOW, same_decisions(a, [run_ref(kind, shape, ls, qo, order)[0] for order in ("fsum", "reversed")]))


def agree(a, b, window):
    """tests/test_gpu_spg.py::_compare's conditions between two runs of the restatement: None, or the first (iteration, what) that breaks them"""
    if len(a.trace) < window or len(b.trace) < window:
        return (min(len(a.trace), len(b.trace)), "length")
    for k in range(window):
        r, q = a.trace[k], b.trace[k]
        if r["n_evals"] != q["n_evals"] or r["ls_iters"] != q["ls_iters"]:
            return (k, "counts")
        if not abs(q["t"] - r["t"]) <= 1e-9 * abs(r["t"]):
            return (k, "t")
        if not np.linalg.norm(b.trace_x[k] - a.trace_x[k]) <= 1e-9 * max(1.0, np.linalg.norm(a.trace_x[k])):
            return (k, "x")
        if not abs(q["gnorm"] - r["gnorm"]) <= 1e-7 * max(1.0, r["gnorm"]):
            return (k, "gnorm")
    return None


# ---- n = 2: every sum has one order, so the device's run is the restatement's bit for bit (with ref_prox.seq_dot) ----
TINY_SEED = 554  # (chosen on the CPU: the first search interpolates, and h1 taken from p instead of the rounded x + d changes the bits of its t)
TINY_ITERS = 12


def tiny_problem(n=2, seed=TINY_SEED):
    """f = 1/2 sum q_j (x_j - c_j)^2: (fn, q, c, x0, l1)"""
    rng = np.random.default_rng(seed)
    q = np.array([1.0, 40.0])[:n] * rng.uniform(0.5, 2.0, 2)[:n]
    c = (rng.standard_normal(2) * 3)[:n]
    x0 = (rng.standard_normal(2) * 5)[:n]

    def fn(x):
        return 0.5 * float(np.sum(q * (x - c) ** 2)), q * (x - c)
    return fn, q, c, x0, np.array([0.3, 0.7])[:n]


def run_tiny(n=2, faults=(), iters=TINY_ITERS):
    fn, _, _, x0, l1 = tiny_problem(n)
    o = R.CountingOracle(fn)
    s = RP.SpectralProximalGradient(1e-12, x0, o, l1, dot=RP.seq_dot, faults=faults)
    try:
        s.minimize(RP.GLLQuadratic(1e-4, 1), o, iters, MAX_LS)
    except R.MaxIterReached:
        pass
    return s


# ---- whole runs ----
@functools.lru_cache(maxsize=None)
def run_problem(kind, m, n):
    """(fn, l1, x0) of a whole-run case: the data is logistic_cases.problem's A (and its labels and weights for the logistic regression)"""
    a, y, w, _, _, _ = LC.problem(m, n)
    l1 = np.full(n, RUN_L1[kind])
    l1[0] = 0.0
    if kind == "logistic":
        return RL.logistic_fn(a, y, w, RUN_MU), l1, np.zeros(n)
    rng = np.random.default_rng(7000 * m + n)
    xs = np.where(rng.random(n) < 0.2, rng.standard_normal(n), 0.0)
    b = a @ xs + 0.1 * rng.standard_normal(m)
    at = np.ascontiguousarray(a.T)

    def fn(x):
        r = a @ x - b
        return 0.5 * float(r @ r) + 0.5 * RUN_MU * float(x @ x), at @ r + RUN_MU * x
    return fn, l1, np.zeros(n)


def run_box(n, boxed):
    return (np.zeros(n), np.full(n, np.inf)) if boxed else (None, None)


@functools.lru_cache(maxsize=None)
def run_whole(kind, m, n, boxed):
    """the restatement to RUN_TOL under GLLQuadratic(1e-4, 10) with numpy.dot: (solver object, status)"""
    fn, l1, x0 = run_problem(kind, m, n)
    lb, ub = run_box(n, boxed)
    o = R.CountingOracle(fn)
    s = RP.SpectralProximalGradient(RUN_TOL, x0, o, l1, lb, ub)
    status = "ok"
    try:
        s.minimize(line_search("gll"), o, RUN_CAP, MAX_LS)
    except R.MaxIterReached:
        status = "max_iter"
    return s, status


# ---- set_l1 between two calls (rule 7): logistic (96, 64), l1 2 -> 1 after 5 iterations.  With the ring kept, the first search at the new penalty
# accepts t = 1 against the old penalty's larger values; with the ring cleared it has to interpolate once ----
RESTART_SHAPE, RESTART_L1, RESTART_K = (96, 64), (2.0, 1.0), 5


@functools.lru_cache(maxsize=None)
def run_restart(clear=True, more=3):
    """(trace of the first call, trace of the call after set_l1)"""
    a, y, w, mu, x0, _ = LC.problem(*RESTART_SHAPE)
    o = R.CountingOracle(RL.logistic_fn(a, y, w, mu))
    s = RP.SpectralProximalGradient(RUN_TOL, x0, o, RESTART_L1[0])
    ls = line_search("gll")
    try:
        s.minimize(ls, o, RESTART_K, MAX_LS)
    except R.MaxIterReached:
        pass
    first = s.trace
    s.set_l1(RESTART_L1[1], ls if clear else None)
    try:
        s.minimize(ls, o, more, MAX_LS)
    except R.MaxIterReached:
        pass
    return first, s.trace
