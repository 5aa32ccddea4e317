"""What tests/test_ref_owlqn.py (CPU) and tests/test_gpu_owlqn.py (GPU) share: the problems of OWLQN's tests, the restatement's runs (each made
once and kept), the windows and the whole runs.

WINDOW CASES: prox_cases' smooth parts and penalties without their boxes, BackTracking(1e-4, 0.5), tol 1e-10:
    quadratic 64, m = 5 and m = 2   L1 least squares, scalar l1 = 0.5 (m = 2: the ring wraps inside the window)
    quadratic 1000                  l1 per entry (0.5, every seventh entry unpenalised)
    logistic (96, 64)               l1 = 2 with the first column unpenalised
    sparse logistic (64, 20000)     scalar l1 = 0.25
    multinomial (40, 13, 5)         l1 = 1 with the first feature of every class unpenalised

THE WINDOW of a case is the number of leading iterations, 30 at the most, over which the restatement takes the same decisions (n_evals, ls_iters
and `updated` of every iteration) under numpy.dot, math.fsum and a reversed-order sum, and under the two-loop recursion and the compact form,
with t and x of all these runs within 1e-11 (relative, as tests/test_ref_lbfgs.py measures it) of the first -- a factor of 100 inside what the
GPU comparison allows -- and while lbfgs_cases.above_f_floor holds on the composite values.  WINDOWS states them;
tests/test_ref_owlqn.py::test_window_self_check computes them again and asserts this table.

WHOLE RUNS: prox_cases.RUN_SHAPES without a box -- L1 logistic regression (l1 = 2) and L1 least squares (l1 = 5) as host closures at (96, 64),
(40, 65), (257, 200), one unpenalised column, mu = 1e-3, x0 = 0, m = 5, BackTracking(1e-4, 0.5) to RUN_TOL.
"""
import functools

import numpy as np

import lbfgs_cases as LBC
import prox_cases as PC
import ref_owlqn as RO
import ref_prox as RP
import ref_spg as R

MAX_WINDOW = 30
TOL = 1e-10
MAX_LS = 50
LICENCE = 1e-11
C1, BETA = 1e-4, 0.5
WINDOW_CASES = [("quadratic", (64,), 5), ("quadratic", (64,), 2), ("quadratic", (1000,), 5), ("logistic", (96, 64), 5),
                ("sparse_logistic", (64, 20000), 5), ("multinomial", (40, 13, 5), 5)]
DOTS = PC.DOTS
VARIANTS = (("fsum", "two_loop"), ("reversed", "two_loop"), ("numpy", "compact"))
# computed by window() on the CPU; asserted by tests/test_ref_owlqn.py::test_window_self_check
# (29: lbfgs_cases.above_f_floor needs f of the iteration behind; sparse logistic: its decrease falls below 1e4 ulp of F at iteration 22)
WINDOWS = {("quadratic", (64,), 5): 29, ("quadratic", (64,), 2): 29, ("quadratic", (1000,), 5): 29, ("logistic", (96, 64), 5): 29,
           ("sparse_logistic", (64, 20000), 5): 22, ("multinomial", (40, 13, 5), 5): 29}

RUN_CASES = [(kind, m, n) for kind in ("logistic", "least_squares") for (m, n) in PC.RUN_SHAPES]
RUN_CAP = 500
# the tightest of 1e-7, 1e-6, 1e-5 the restatement reaches under all three summation orders on every case (run_tol() computes it again)
RUN_TOL = 1e-5
# the largest |x_owlqn - x_prox| (infinity norm) over RUN_CASES, both restatements at RUN_TOL with numpy.dot (run_gap() computes it again)
RUN_GAP = 1.2387178298878254e-05  # (least squares (40, 65); the other five cases: 3.2e-8 to 7.2e-6)


def line_search():
    return RO.BackTracking(C1, BETA)


def l1_of(kind, shape):
    return PC.l1_of(kind, shape)


_runs = {}


def run_ref(kind, shape, m, qo=None, order="numpy", direction="two_loop", iters=MAX_WINDOW, faults=()):
    """The restatement on one window case: (solver object, oracle, status); kept"""
    key = (kind, shape, m, order, direction, iters, tuple(faults))
    if key not in _runs:
        fn, x0 = PC.smooth(kind, shape, qo)
        o = R.CountingOracle(fn)
        s = RO.OWLQN(TOL, x0, l1_of(kind, shape), m=m, dot=DOTS[order], direction=direction, faults=faults)
        status = "ok"
        try:
            s.minimize(line_search(), o, iters, MAX_LS)
        except R.MaxIterReached:
            status = "max_iter"
        except RO.AbnormalTermination:
            status = "abnormal"
        _runs[key] = (s, o, status)
    return _runs[key]


def same_decisions(a, others):
    w = min([len(a.trace)] + [len(o.trace) for o in others])
    for k in range(w):
        for o in others:
            if any(a.trace[k][key] != o.trace[k][key] for key in ("n_evals", "ls_iters", "updated")):
                return k
    return w


def spread(a, o, k):
    """tests/test_ref_lbfgs.py::_spread at one iteration"""
    return max(float(np.linalg.norm(a.trace_x[k] - o.trace_x[k]) / max(1.0, np.linalg.norm(a.trace_x[k]))),
               abs(a.trace[k]["t"] - o.trace[k]["t"]) / abs(a.trace[k]["t"]))


def window(kind, shape, m, qo=None):
    a = run_ref(kind, shape, m, qo)[0]
    others = [run_ref(kind, shape, m, qo, order, direction)[0] for order, direction in VARIANTS]
    w = min(MAX_WINDOW, same_decisions(a, others), LBC.above_f_floor(a, "bt"))
    for k in range(w):
        if any(spread(a, o, k) > LICENCE for o in others):
            return k
    return w


def agree(a, b, window):
    """tests/test_gpu_spg.py::_compare's conditions between two runs: None, or the first (iteration, what) that breaks them"""
    return PC.agree(a, b, window)


# ---- n = 1 and 2: every sum has one order, so the device's first iteration (no pair: z = v) is the restatement's bit for bit ----
def tiny_problem(n):
    """f = 1/2 sum q_j (x_j - c_j)^2: (fn, x0, l1).  Entry 0 starts at 5e-4 with v_0 = 10.3005: the unit step crosses zero and is projected onto 0.0,
    so v.(xt - x) = -5.15e-3 while t v.d = -106.  F_t - F_k = -5.15e-3 passes rule 6 and fails c1 t v.d = -1.06e-2: with Armijo's right side the
    first search halves, with Andrew and Gao's it accepts t = 1.  Entry 1 starts 1e-3 from its own minimiser and hardly moves."""
    q, c = np.array([1.0, 1.0])[:n], np.array([-10.0, 3.0])[:n]

    def fn(x):
        return 0.5 * float(np.sum(q * (x - c) ** 2)), q * (x - c)
    return fn, np.array([5e-4, 2.301])[:n], np.array([0.3, 0.7])[:n]


def run_tiny(n, iters=1, faults=()):
    fn, x0, l1 = tiny_problem(n)
    o = R.CountingOracle(fn)
    s = RO.OWLQN(1e-12, x0, l1, dot=RP.seq_dot, faults=faults)
    try:
        s.minimize(line_search(), o, iters, MAX_LS)
    except R.MaxIterReached:
        pass
    return s


# ---- whole runs ----
@functools.lru_cache(maxsize=None)
def run_whole(kind, m, n, tol=None, order="numpy"):
    """the restatement to `tol` (RUN_TOL): (solver object, status)"""
    fn, l1, x0 = PC.run_problem(kind, m, n)
    o = R.CountingOracle(fn)
    s = RO.OWLQN(RUN_TOL if tol is None else tol, x0, l1, m=5, dot=DOTS[order])
    status = "ok"
    try:
        s.minimize(line_search(), o, RUN_CAP, MAX_LS)
    except R.MaxIterReached:
        status = "max_iter"
    except RO.AbnormalTermination:
        status = "abnormal"
    return s, status


@functools.lru_cache(maxsize=None)
def run_whole_prox(kind, m, n, tol=None):
    """ref_prox.SpectralProximalGradient + GLLQuadratic(1e-4, 10) on the same problem to the same tolerance: (solver object, status)"""
    tol = RUN_TOL if tol is None else tol
    if tol == PC.RUN_TOL:
        return PC.run_whole(kind, m, n, False)
    fn, l1, x0 = PC.run_problem(kind, m, n)
    o = R.CountingOracle(fn)
    s = RP.SpectralProximalGradient(tol, x0, o, l1)
    status = "ok"
    try:
        s.minimize(PC.line_search("gll"), o, PC.RUN_CAP, PC.MAX_LS)
    except R.MaxIterReached:
        status = "max_iter"
    return s, status


def run_tol():
    for tol in (1e-7, 1e-6, 1e-5):
        if all(run_whole(*case, tol=tol, order=order)[1] == "ok" for case in RUN_CASES for order in DOTS):
            return tol
    return None


def run_gap():
    return max(float(np.max(np.abs(run_whole(*case)[0].x - run_whole_prox(*case)[0].x))) for case in RUN_CASES)


# ---- warm restart and set_l1 between calls (rule 9): logistic (96, 64), l1 2 -> 1 ----
RESTART_SHAPE, RESTART_L1, RESTART_K = (96, 64), (2.0, 1.0), 6


def restart_problem():
    import logistic_cases as LC
    import ref_logistic as RL
    a, y, w, mu, x0, _ = LC.problem(*RESTART_SHAPE)
    return (a, y, w, mu), RL.logistic_fn(a, y, w, mu), x0


# ---- the replay's cases (tests/owlqn_replay.py; licensed by tests/test_ref_owlqn.py, run on the GPU by tests/test_gpu_owlqn_replay.py) ----
REPLAY_L1 = 5.0
REPLAY_TOL = 1e-10


def shifted_separable(n, kappa=None):
    """f = sum_i (a_i/2 (x_i - c_i)^2 + 1/4 (x_i - c_i)^4), a_i in [1, 100] and c_i in [-1, 1] on fixed patterns (lbfgs_cases.separable_problem moved
    off the origin): with l1 = 5 the entries with a_i |c_i| + |c_i|^3 <= 5 end at exactly 0, the others on either side of it.  `kappa`: a_i spread
    geometrically over [1, kappa] instead ("hard": at kappa = 1e6, m = 32 and n = 64 the restatement is still taking steps the replay can tell
    apart after 72 iterations; on [1, 100] it has converged after 25, before the ring is full)"""
    i = np.arange(n, dtype=np.float64)
    a = 1.0 + 99.0 * ((i * 0.6180339887498949) % 1.0) if kappa is None else kappa ** ((i * 0.6180339887498949) % 1.0)
    c = 2.0 * ((i * 0.7548776662466927 + 0.3) % 1.0) - 1.0
    x0 = 0.5 + ((i * 0.3819660112501051) % 1.0)

    def fn(x):
        e = x - c
        e2 = e * e
        return float(np.sum(0.5 * a * e2 + 0.25 * e2 * e2)), a * e + e2 * e
    return fn, x0


def _replay_case(name, prob, n, m, iters, calls=1):
    return dict(name=name, prob=prob, n=n, m=m, iters=iters, calls=calls)


REPLAY_CASES = ([_replay_case(f"wrap-m{m}-n{n}", "sep", n, m, 2 * (m + 1) + 4) for m in (1, 2, 5) for n in (7, 2050)]
                + [_replay_case("m32-n64", "hard", 64, 32, 72)]                 # the ring full and wrapping
                + [_replay_case("warm-restart", "sep", 2050, 5, 20, calls=2)])  # 2 x 20 iterations replayed as one


def replay_problem(case):
    """(fn, x0, l1) of a replay case"""
    fn, x0 = shifted_separable(case["n"], 1e6 if case["prob"] == "hard" else None)
    return fn, x0, REPLAY_L1


def replay_ref(case, dot=np.dot):
    """the float64 restatement of a replay case as an owlqn_replay.Run"""
    import owlqn_replay as OR
    fn, x0, l1 = replay_problem(case)
    rec = OR.Recorder(fn)
    o = R.CountingOracle(rec)
    s = RO.OWLQN(REPLAY_TOL, x0, l1, m=case["m"], dot=dot)
    run = OR.Run(case["m"], False, l1, x0, rec)
    for _ in range(case["calls"]):
        states = []
        try:
            s.minimize(line_search(), o, case["iters"], MAX_LS, callback=lambda r: states.append((r.stored_pairs(), r.gamma, r.resets)))
        except R.MaxIterReached:
            pass
        # gamma() after iteration k is the scaling of direction k: the state seen in the callback
        run.extend(s.trace_x, [r["t"] for r in s.trace], s.updated, states)
    return run
