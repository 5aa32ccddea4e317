"""Pure-Python (numpy float64) restatement of the ExactQuadratic line search (QN_LS_EXACT_QUADRATIC, kernels csrc/qn_vec_exact.hip.h) on the loops of
tests/ref_spg.py (SPG, projected gradient), tests/ref_lbfgs.py (L-BFGS, free and in a box) and tests/ref_cg.py (NonlinearCG).  Those solvers are used
as they are -- their compute_direction and update_next_iterate -- through two objects that share one state:

    ExactOracle      stands where the loops call `oracle(x)`.  It hands out the evaluation the search left at the accepted point (the recurrence's or
                     the objective's) when it is asked for exactly that point, and calls the objective otherwise.  `evals` counts the objective's calls.
    ExactQuadratic   compute_step_len: the search, operation for operation as the device runs it:
                       1. gd = g.d; unless gd < 0: NotDescent
                       2. q = Q d, c = d.q
                       3. unless c > 0 and finite: NonPositiveCurvature
                       4. t = (-gd) / c; with a box t = min(t, 1) as a comparison
                       5. xt = x + t d
                       6. refresh iteration: (f_t, gt) = the objective at xt; otherwise gt = g + t q, f_t = f + t (gd + (0.5 t) c)
                       7. accepted

and `minimize`, ref_spg._Base.minimize restated with the one rule that loop does not have: convergence is declared only on a gradient the objective
evaluated -- when the test passes on a recurrence gradient, x is evaluated by the objective (a forced refresh, counted) and the loop top runs again.

Refresh rule, r = refresh_every: r = 1 every accepted point is evaluated by the objective; r = k > 1 every k-th (`since` counts accepted points since
the objective last evaluated one, and survives calls); r = 0 never.  `dot=` is a parameter as in ref_spg.py; the product Q d is `hess_vec`.
Test infrastructure: the product does not import this file."""
import math

import numpy as np

import ref_spg as R


class NotDescent(Exception):
    pass


class NonPositiveCurvature(Exception):
    pass


class ExactOracle:
    def __init__(self, fn, hess_vec, refresh_every=1):
        self.fn, self.hess_vec, self.r = fn, hess_vec, refresh_every
        self.calls = self.evals = 0
        self.memo = None          # (x, f, g) of the accepted point
        self.g_true = False       # the evaluation last handed out is the objective's own
        self.since = 0
        self.refreshes = self.forced = self.passes = 0

    def evaluate(self, x):
        self.evals += 1
        f, g = self.fn(np.array(x, dtype=np.float64))
        return float(f), np.asarray(g, dtype=np.float64)

    def __call__(self, x):
        self.calls += 1
        if self.memo is not None and np.array_equal(self.memo[0], x):
            return self.memo[1], self.memo[2]
        f, g = self.evaluate(x)
        self.memo, self.g_true, self.since = (np.array(x, dtype=np.float64), f, g), True, 0
        return f, g

    def force(self, x):
        """the loop top's test passed on a recurrence gradient: the objective evaluates x"""
        self.memo = None
        self.refreshes += 1
        self.forced += 1
        return self(x)


class ExactQuadratic:
    def __init__(self, oracle, bounded=False, dot=np.dot):
        self.o, self.bounded, self.dot = oracle, bounded, dot
        self.trials = 0
        self.history = []  # per search: dict(t, c, gd, capped, refresh)

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):
        o = self.o
        f_k, g_k = eval_x_k
        gd = float(self.dot(g_k, direction_k))
        if not gd < 0.0:
            raise NotDescent()
        q = o.hess_vec(direction_k)
        c = float(self.dot(direction_k, q))
        o.passes += 1
        if not c > 0.0 or math.isinf(c):
            raise NonPositiveCurvature()
        t = (-gd) / c
        capped = False
        if self.bounded and t > 1.0:
            t, capped = 1.0, True
        xt = x_k + t * direction_k
        refresh = o.r == 1 or (o.r > 1 and o.since + 1 >= o.r)
        if refresh:
            f_t, gt = o.evaluate(xt)
            o.since, o.g_true = 0, True
            o.refreshes += 1
        else:
            gt = g_k + t * q
            f_t = f_k + t * (gd + (0.5 * t) * c)
            o.since += 1
            o.g_true = False
        o.memo = (xt, f_t, gt)
        self.history.append(dict(t=t, c=c, gd=gd, capped=capped, refresh=refresh))
        return t


def minimize(solver, line_search, oracle, max_iter_solver):
    """ref_spg._Base.minimize with the convergence rule.  Returns "ok"; raises ref_spg.MaxIterReached, NotDescent, NonPositiveCurvature."""
    solver.k = 0
    solver.trace, solver.trace_x = [], []
    while max_iter_solver > solver.k:
        eval_x_k = oracle(solver.x)
        if math.isnan(eval_x_k[0]) or math.isinf(eval_x_k[0]):
            raise R.OutOfDomain()
        if solver.has_converged(eval_x_k):
            if not oracle.g_true:
                eval_x_k = oracle.force(solver.x)
                if solver.has_converged(eval_x_k):
                    return "ok"
            else:
                return "ok"
        direction = solver.compute_direction(eval_x_k)
        gnorm = float(np.max(np.abs(solver.projected_gradient(eval_x_k))))
        t = solver.update_next_iterate(line_search, eval_x_k, oracle, direction, 0)
        solver.trace.append(dict(f=eval_x_k[0], gnorm=gnorm, t=t, s_norm=getattr(solver, "last_s_norm", 0.0)))
        solver.trace_x.append(solver.x.copy())
        solver.k += 1
    raise R.MaxIterReached()
