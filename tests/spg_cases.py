"""The problems the first-order solvers' tests share (tests/test_ref_spg.py justifies the windows, tests/test_gpu_spg.py uses them): the
seeded synthetic quadratic of tests/problems.py with kappa = 1e2, SPG + GLLQuadratic(1e-4, 10) and PGD + BackTrackingB(1e-4, 0.5), a box of
+-0.05 and an infinite one."""
import numpy as np

import problems as P
import ref_spg as R

KAPPA = 1e2
WINDOW = 30  # iterations compared; tests/test_ref_spg.py::test_summation_order_self_check licenses it for every case below
SIZES = (64, 512, 1000, 2048)  # (1000: not a multiple of 128)
BOXES = (0.05, float("inf"))
SOLVERS = ("spg_gll", "pgd_btb")
CASES = [(s, n, box) for s in SOLVERS for n in SIZES for box in BOXES]
BIG_N = 4096  # through Quadratic.synthetic


def problem(qo, n):
    diag = P.synth_diag(n, KAPPA)
    q = qo.synth_rows(n, 0, n, P.SEED, diag)
    b, x0 = P.synth_vectors(n, P.SEED)
    return q, b, x0, diag


def chain_problem(n=1000, seed=5):
    """The double-well chain of examples/device_closure.hip (tests/test_gpu_device_closure.py's problem), box +-1.5."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 2.0, n)
    x0 = rng.uniform(-2.0, 2.0, n)
    return a, 0.3, x0, np.full(n, -1.5), np.full(n, 1.5)


def chain_fn(a, c):
    def fn(x):
        w = x * x - a
        d = np.diff(x)
        g = x * w
        g[:-1] -= c * d
        g[1:] += c * d
        return 0.25 * np.sum(w * w) + 0.5 * c * np.sum(d * d), g
    return fn


def lse_problem(m=96, n=64, seed=3):
    """f = log sum_i exp(a_i'x + c_i) + mu/2 ||x||^2 at a small size, box +-0.3."""
    rng = np.random.default_rng(seed)
    a, c, mu = rng.standard_normal((m, n)), rng.standard_normal(m), 0.5
    x0 = rng.standard_normal(n)
    return a, c, mu, x0, np.full(n, -0.3), np.full(n, 0.3)


def lse_fn(a, c, mu):
    def fn(x):
        z = a @ x + c
        zm = z.max()
        w = np.exp(z - zm)
        sw = w.sum()
        return zm + np.log(sw) + 0.5 * mu * (x @ x), a.T @ (w / sw) + mu * x
    return fn


def bounds(n, box):
    return np.full(n, -box), np.full(n, box)


def run_ref(solver, fn, x0, lb, ub, iters, dot=np.dot, max_ls=50, memo_calls=False):
    """The restatement on one case: (solver object, oracle).  Raises nothing on the iteration cap."""
    o = R.CountingOracle(fn)
    if solver == "spg_gll":
        s = R.SpectralProjectedGradient(1e-10, x0, o, lb, ub, dot=dot)
        ls = R.GLLQuadratic(1e-4, 10, dot=dot)
    else:
        s = R.ProjectedGradientDescent(1e-10, x0, lb, ub)
        ls = R.BackTrackingB(1e-4, 0.5, lb, ub, dot=dot)
    try:
        s.minimize(ls, o, iters, max_ls)
    except R.MaxIterReached:
        pass
    return s, o
