"""Pure-Python (float64) restatement of the StrongWolfe line search of the vector-machine solvers (QN_LS_STRONG_WOLFE, kernels
csrc/qn_vec_wolfe.hip.h): MINPACK-2 `dcsrch` / `dcstep` (More' and Thuente, ACM TOMS 20, 1994) on tests/ref_spg.py's `compute_step_len`
interface -- one oracle call per trial, the bracket's (f, f') kept.  `dot=` is a parameter as in ref_spg.py.

    ftol = c1, gtol = c2, xtol, stpmin = t_min, stpmax = t_max; the first trial is min(max(1, stpmin), stpmax)
    the boxed form (lower_bound / upper_bound given): stpmax = min(t_max, min_i ratio_i) per search (the ratio of morethuente_b.rs:185-197),
    never written back into t_max

Two rules `dcsrch` does not have, shared with the kernels:
    * a trial whose f or phi' is not finite counts as "sufficient decrease fails, derivative positive": none of the tests that need f passes,
      the bracket becomes [stx, stp] and the next trial bisects it; the end point's f is remembered as not finite, and the one `dcstep` case
      that interpolates through the far end point (case 4, bracketed) bisects instead while that is so.  Digit 5 in `ls_cases`.
    * g.d >= 0 (or NaN) at the start: `NotDescent` (the GPU: QN_ABNORMAL_TERMINATION, x stays at x_k).
max / min / clip are written as comparisons (`a if a > b else b`) so that the kernels can state the same operations.
Test infrastructure: the product does not import this file.
"""
import math

import numpy as np

import ref_spg as R

LS_MODIFIED = 1 << 30  # QN_TRACE_LS_MODIFIED: here, the switch to the second stage was thrown in this search


class NotDescent(Exception):
    pass


def seq_dot(a, b):
    """the products added one after the other from 0.0, two roundings each: what one GPU thread does at n = 2"""
    acc = 0.0
    for u, v in zip(np.asarray(a, dtype=np.float64).tolist(), np.asarray(b, dtype=np.float64).tolist()):
        acc = acc + u * v
    return acc


def _mx(a, b):
    return a if a > b else b


def _mn(a, b):
    return a if a < b else b


def _sign(v):
    return (1.0 if v > 0.0 else 0.0) - (1.0 if v < 0.0 else 0.0)


def dcstep(stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax):
    """-> (stx, fx, dx, sty, fy, dy, stp, brackt, case)"""
    sgnd = _sign(dp) * _sign(dx)
    if fp > fx:  # case 1: a higher function value; the minimum is bracketed
        case = 1
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = _mx(_mx(abs(theta), abs(dx)), abs(dp))
        gamma = s * math.sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s))
        if stp < stx:
            gamma = -gamma
        p = (gamma - dx) + theta
        q = ((gamma - dx) + gamma) + dp
        r = p / q
        stpc = stx + r * (stp - stx)
        stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
        stpf = stpc if abs(stpc - stx) <= abs(stpq - stx) else stpc + (stpq - stpc) / 2.0
        brackt = True
    elif sgnd < 0.0:  # case 2: lower function value, derivatives of opposite sign; bracketed
        case = 2
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = _mx(_mx(abs(theta), abs(dx)), abs(dp))
        gamma = s * math.sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = ((gamma - dp) + gamma) + dx
        r = p / q
        stpc = stp + r * (stx - stp)
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
        brackt = True
    elif abs(dp) < abs(dx):  # case 3: lower value, same sign, the derivative's magnitude decreases
        case = 3
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = _mx(_mx(abs(theta), abs(dx)), abs(dp))
        v = (theta / s) * (theta / s) - (dx / s) * (dp / s)
        gamma = s * math.sqrt(v if v > 0.0 else 0.0)
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = (gamma + (dx - dp)) + gamma
        r = p / q
        if r < 0.0 and gamma != 0.0:
            stpc = stp + r * (stx - stp)
        elif stp > stx:
            stpc = stpmax
        else:
            stpc = stpmin
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        if brackt:
            stpf = stpc if abs(stpc - stp) < abs(stpq - stp) else stpq
            lim = stp + 0.66 * (sty - stp)
            stpf = _mn(lim, stpf) if stp > stx else _mx(lim, stpf)
        else:
            stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
            stpf = _mn(stpmax, stpf)
            stpf = _mx(stpmin, stpf)
    else:  # case 4: lower value, same sign, the derivative's magnitude does not decrease
        case = 4
        if brackt:
            if math.isfinite(fy):
                theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
                s = _mx(_mx(abs(theta), abs(dy)), abs(dp))
                gamma = s * math.sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s))
                if stp > sty:
                    gamma = -gamma
                p = (gamma - dp) + theta
                q = ((gamma - dp) + gamma) + dy
                r = p / q
                stpf = stp + r * (sty - stp)
            else:  # (the far end point was a non-finite trial: no cubic through it)
                stpf = stp + 0.5 * (sty - stp)
        elif stp > stx:
            stpf = stpmax
        else:
            stpf = stpmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0.0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    return stx, fx, dx, sty, fy, dy, stpf, brackt, case


class Dcsrch:
    """`dcsrch` between two oracle calls: start() gives the first trial, step(f, g) the verdict on the trial just evaluated."""

    def __init__(self, ftol, gtol, xtol, stpmin, stpmax):
        self.ftol, self.gtol, self.xtol, self.stpmin, self.stpmax = ftol, gtol, xtol, stpmin, stpmax

    def start(self, finit, ginit):
        if not ginit < 0.0:
            raise NotDescent("INITIAL G .GE. ZERO")
        if self.stpmax < self.stpmin:
            raise NotDescent("STPMAX .LT. STPMIN")
        self.brackt, self.stage, self.switched = False, 1, False
        self.finit, self.ginit = finit, ginit
        self.gtest = self.ftol * ginit
        self.width = self.stpmax - self.stpmin
        self.width1 = self.width / 0.5
        self.stx, self.fx, self.gx = 0.0, finit, ginit
        self.sty, self.fy, self.gy = 0.0, finit, ginit
        self.stp = _mn(_mx(1.0, self.stpmin), self.stpmax)
        self.stmin = 0.0
        self.stmax = self.stp + 4.0 * self.stp
        return self.stp

    def step(self, f, g):
        """-> (task, case): task "CONVERGENCE" / "WARNING: ..." (self.stp is the step just evaluated) or "FG" (self.stp is the next trial);
        case 1..4 (dcstep), 5 (a non-finite trial), 0 (the search returned)"""
        stp = self.stp
        bad = not (math.isfinite(f) and math.isfinite(g))
        ftest = self.finit + stp * self.gtest
        if self.stage == 1 and not bad and f <= ftest and g >= 0.0:
            self.stage, self.switched = 2, True
        task = None
        if self.brackt and (stp <= self.stmin or stp >= self.stmax):
            task = "WARNING: ROUNDING ERRORS PREVENT PROGRESS"
        if self.brackt and self.stmax - self.stmin <= self.xtol * self.stmax:
            task = "WARNING: XTOL TEST SATISFIED"
        if not bad and stp == self.stpmax and f <= ftest and g <= self.gtest:
            task = "WARNING: STP = STPMAX"
        if stp == self.stpmin and (bad or f > ftest or g >= self.gtest):
            task = "WARNING: STP = STPMIN"
        if not bad and f <= ftest and abs(g) <= self.gtol * (-self.ginit):
            task = "CONVERGENCE"
        if task is not None:
            return task, 0
        if bad:
            case = 5
            self.brackt = True
            self.sty, self.fy, self.gy = stp, math.inf, -self.ginit
            stp = self.stx + 0.5 * (stp - self.stx)
        elif self.stage == 1 and f <= self.fx and f > ftest:  # the modified function psi
            gt = self.gtest
            fm, fxm, fym = f - stp * gt, self.fx - self.stx * gt, self.fy - self.sty * gt
            gm, gxm, gym = g - gt, self.gx - gt, self.gy - gt
            self.stx, fxm, gxm, self.sty, fym, gym, stp, self.brackt, case = dcstep(self.stx, fxm, gxm, self.sty, fym, gym, stp, fm, gm, self.brackt,
                                                                                      self.stmin, self.stmax)
            self.fx, self.fy = fxm + self.stx * gt, fym + self.sty * gt
            self.gx, self.gy = gxm + gt, gym + gt
        else:
            self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, self.brackt, case = dcstep(self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp,
                                                                                                     f, g, self.brackt, self.stmin, self.stmax)
        if self.brackt:
            if abs(self.sty - self.stx) >= 0.66 * self.width1:
                stp = self.stx + 0.5 * (self.sty - self.stx)
            self.width1 = self.width
            self.width = abs(self.sty - self.stx)
            self.stmin, self.stmax = _mn(self.stx, self.sty), _mx(self.stx, self.sty)
        else:
            self.stmin = stp + 1.1 * (stp - self.stx)
            self.stmax = stp + 4.0 * (stp - self.stx)
        stp = _mx(stp, self.stpmin)
        stp = _mn(stp, self.stpmax)
        if (self.brackt and (stp <= self.stmin or stp >= self.stmax)) or (self.brackt and self.stmax - self.stmin <= self.xtol * self.stmax):
            stp = self.stx
        self.stp = stp
        return "FG", case


class StrongWolfe:
    def __init__(self, c1=1e-4, c2=0.9, xtol=0.1, t_min=0.0, t_max=1e10, lower_bound=None, upper_bound=None, dot=np.dot):
        assert 0.0 < c1 < c2 < 1.0
        self.c1, self.c2, self.xtol, self.t_min, self.t_max, self.dot = c1, c2, xtol, t_min, t_max, dot
        self.lb = None if lower_bound is None else np.asarray(lower_bound, dtype=np.float64)
        self.ub = None if upper_bound is None else np.asarray(upper_bound, dtype=np.float64)
        self.history = []  # one record per search

    def stpmax_of(self, x_k, d):
        if self.lb is None and self.ub is None:
            return self.t_max
        n = len(x_k)
        lb = self.lb if self.lb is not None else np.full(n, -R.INF)
        ub = self.ub if self.ub is not None else np.full(n, R.INF)
        with np.errstate(all="ignore"):
            ratio = np.where(d > 0.0, (ub - x_k) / d, np.where(d < 0.0, (lb - x_k) / d, R.INF))
        acc = R.INF
        for v in ratio.tolist():  # .fold(INFINITY, |acc, x| x.min(acc))
            acc = R.rmin(v, acc)
        return R.rmin(self.t_max, acc)

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter):
        f_k, g_k = eval_x_k
        gd = float(self.dot(g_k, direction_k))
        rec = dict(finit=f_k, ginit=gd, steps=[], cases=[], ls_cases=0, evaluated=False, task=None, switched=False,
                   x_k=np.array(x_k, dtype=np.float64), d=np.array(direction_k, dtype=np.float64), g_k=np.array(g_k, dtype=np.float64))
        rec["stpmax"] = self.stpmax_of(np.asarray(x_k, dtype=np.float64), np.asarray(direction_k, dtype=np.float64))
        self.history.append(rec)
        self.trials = 0
        m = Dcsrch(self.c1, self.c2, self.xtol, self.t_min, rec["stpmax"])
        t = m.start(f_k, gd)
        i = 0
        while max_iter > i:
            f_t, g_t = oracle(x_k + t * direction_k)
            self.trials += 1
            dphi = float(self.dot(g_t, direction_k))
            rec["steps"].append((t, f_t, dphi))
            task, case = m.step(f_t, dphi)
            if len(rec["cases"]) < 10:
                rec["ls_cases"] += case * 8 ** len(rec["cases"])
            rec["cases"].append(case)
            if m.switched:
                rec["ls_cases"] |= LS_MODIFIED
                rec["switched"] = True
            if task != "FG":
                rec["evaluated"], rec["task"], rec["t"] = True, task, t
                return t
            t = m.stp
            i += 1
        rec["t"] = t
        return t
