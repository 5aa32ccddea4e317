"""Replay of a run of the base family of the device-wide vector machine -- QN_SPG, QN_PROJECTED_GRADIENT, QN_PROJECTED_NEWTON,
QN_SPECTRAL_PROJECTED_NEWTON with GLLQuadratic, BackTracking and BackTrackingB (kernels vec_dir, vec_top, vec_trial, vec_decide, vec_accept,
vec_post and pn_small of csrc/qn_vec.hip.h) -- step by step, from the outside (tests/test_ref_vec_replay.py licenses it on the float64
restatements, tests/test_gpu_vec_replay.py applies it to the GPU; cases in tests/vec_replay_cases.py).  Test infrastructure: the product does
not import this file.

WHAT IS KNOWN.  The settings, P(x0), a host closure that records every point it was asked and what it answered, in order
(lbfgs_replay.Recorder), and per iteration what a `minimize` callback reads (direction(), lambda_(), s_norm() / y_norm()) plus the trace with
x.  Every iteration is checked ON ITS OWN from (x_k, g_k, lambda_k): nothing accumulates.

BIT FOR BIT (+0.0 and -0.0 equal; fmax / fmin return the non-NaN operand, as the device's do).  The element-wise operations round once each,
in a stated order, with no fused multiply-add, and numpy restates them:
  1. d_k = fmin(fmax(x - lam g, lb), ub) - x, the product first (PGD: no lam; the Newton pair: z = H^-1 g for g, item 9).
  2. trace gnorm = max |pg| with the exact comparisons x == lb && g > 0, x == ub && g < 0.
  3. trace f = the closure's f(x_k).
  4. trial points x + t d (t d first), projected onto the LINE SEARCH'S box under BackTrackingB; the accepted trial and x_{k+1} with the
     trace's t; x_{k+1} is x + t d, never the projected trial.
  5. the sequence of points handed to the closure: loop top, trials, the evaluation at x_{k+1} where the method needs y (memoize 0: and the
     next loop top again); n_evals, ls_iters, oracle_calls and oracle_evals with it.
  6. the GLL ring: f_max is the maximum of the last m loop-top values, carried across minimize calls (seen through the decisions it takes).

INSIDE DERIVED BOUNDS.  Truth is np.longdouble, chunk by chunk (lbfgs_replay.cross).  A sum of n products in any order, with or without FMA,
is off by at most GAMMA(n) sum |a_i b_i|, GAMMA(n) = 1.001 (n + 2) 2^-53 (the count tests/quad_replay_cases.py states).  Every check is a
ratio |error| / bound, asserted <= 1.
  7. the line search on intervals: g.d (and BackTrackingB's diff2) is known to its bound, so every decision is evaluated at both ends; one
     whose ends disagree is UNDECIDABLE.  The decisions' right-hand sides ((c1 t) gd, (-c1 / t) diff2) hold each uncertain operand once, and
     rounding is monotone: the float64 evaluation at the corners bounds the device's.  t_tmp = -0.5 t^2 gd / (ft - fk - t gd) is monotone in
     gd while its denominator's interval excludes 0, and in t while 2 (ft - fk) - t gd keeps its sign; it is evaluated at the corners in
     longdouble and widened by the five roundings of the device's evaluation, (6 + 2 |t gd| / |den|) 2^-53 relative (the subtraction in the
     denominator amplifies the product's rounding).  A rejected trial's t is not visible: the recorded point is held to the element-wise
     interval between fl(x + fl(t_lo d)) and fl(x + fl(t_hi d)).  The trace's t lies in the final interval.
  8. lambda_{k+1}: s.y <= 0 -> lambda_max where |s.y| clears its bound (else undecidable), otherwise clamp(ss / sy) with the quotient's bound
     from both sums and the division; trace s_norm = sqrt(ss); ProjectedNewton's s_norm(), y_norm(), and its stop rule in that order.
  9. z = H^-1 g.  n <= 5: pn_small_kernel is nalgebra operation for operation, so d_k is bit for bit with ref_pnewton._nalgebra_cholesky and
     the substitutions restated here with sequential sums.  Above 5 the projection is nonexpansive, so
         ||d_k - d(z*)||_2 <= lam ||H^-1||_2 ||r||_2 + 4 2^-53 (||x||_2 + lam ||z*||_2),
     z* the extended-precision solve, ||r||_2 <= sqrt(n) B(n) (||H||_inf ||z*||_inf (1 + 1e-3) + ||g||_inf) from the backward error B(n) =
     newton_solve_cases.bound(n) that tests/test_gpu_newton_solve.py asserts.  THIS IS THE ONLY NORM-WISE CHECK IN THIS FILE.

DISCRIMINATION.  An iteration is SKIPPED when a bound says nothing: the t interval wider than 1e-6 t, or lambda's wider than 1e-6 lambda.
"""
import math

import numpy as np

import lbfgs_replay as LR
from lbfgs_replay import LD, cross

U = 2.0 ** -53
INF = float("inf")
CAP = 1e-6
SMALL_N = 5


def gamma(n):
    return LD(1.001 * (n + 2) * U)


def key(x):
    return LR.Recorder._key(x)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and (a + 0.0).tobytes() == (b + 0.0).tobytes()


def first_diff(a, b):
    j = np.flatnonzero((np.asarray(a) + 0.0).view(np.int64) != (np.asarray(b) + 0.0).view(np.int64))
    return int(j[0]) if j.size else -1


# ---- the device's element-wise operations, restated ----
def project(u, lo, hi):
    return np.fmin(np.fmax(u, lo), hi)


def direction(x, w, lam, lb, ub):
    return project(x - (w if lam is None else lam * w), lb, ub) - x


def pg_norm(x, g, lb, ub):
    p = np.where(((x == lb) & (g > 0.0)) | ((x == ub) & (g < 0.0)), 0.0, g)
    return float(np.fmax.reduce(np.abs(p), initial=0.0))


def step(x, t, d):
    return x + t * d


def clamp(v, lo, hi):
    return float(np.fmax(np.fmin(v, hi), lo))


def small_solve(h, g):
    """pn_small_kernel: ref_pnewton's column Cholesky, then both substitutions with sequential sums"""
    import ref_pnewton as RP
    l = RP._nalgebra_cholesky(h)

    def seq(a, b):
        acc = 0.0
        for u, v in zip(a.tolist(), b.tolist()):
            acc = acc + u * v
        return acc
    return RP._nalgebra_solve(l, g, seq)


class HRecorder(LR.Recorder):
    """fn(x) -> (f, g, H).  `wrap(f, g, h, hessian_read)` builds what the solver is handed: the restatements take ref_pnewton.Eval, the Python
    mirror a FuncEvalMultivariate whose hessian() calls `hessian_read`.  The mirror asks the closure a second time, at the same point, for
    the Hessian alone; that call is no evaluation of the run's sequence: when hessian() is read it is taken out of `order` and `calls` and
    its point is kept in `hessian_keys`, which the replay compares with the x_k of the iterations (one factorisation each)."""

    def __init__(self, fn, wrap):
        super().__init__(lambda x: fn(x)[:2], keep_x=True)
        self.full, self.wrap, self.hess, self.hessian_keys = fn, wrap, {}, []

    def __call__(self, x):
        f, g = super().__call__(x)
        k = self.order[-1]
        if k not in self.hess:
            self.hess[k] = self.full(np.array(x, dtype=np.float64))[2]
        idx = len(self.order) - 1
        return self.wrap(f, g, self.hess[k], lambda: self._hessian_read(idx, k))

    def _hessian_read(self, idx, k):
        assert idx == len(self.order) - 1 and self.order[idx] == k, "the Hessian was read from an evaluation that is not the last one"
        self.order.pop()
        self.calls -= 1
        self.hessian_keys.append(k)


class Run:
    """settings and records of one solver over one or more minimize calls.
    method: "spg" | "pgd" | "pn" | "spn";  ls: dict(kind="gll" | "bt" | "btb", c1, m, sigma1, sigma2, beta, lo, hi)
    limited: a device objective -- only d_k, gnorm, x_{k+1} and the update scalars, with g_k as read back (`grads`)."""

    def __init__(self, method, ls, lb, ub, x0, rec, memoize, max_ls, tol, lam_min=1e-3, lam_max=1e3, limited=False):
        self.method, self.ls, self.rec, self.memoize, self.max_ls, self.tol = method, ls, rec, int(memoize), max_ls, tol
        self.lb, self.ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
        self.x0 = project(np.asarray(x0, dtype=np.float64), self.lb, self.ub)
        self.lam_min, self.lam_max, self.lam0, self.limited, self.ctor_lams = lam_min, lam_max, None, limited, (1e-3, 1e3)
        self.calls, self.grads = [], []
        self.hessian_calls = False  # the Python mirror: one Hessian callback per iteration, at x_k (HRecorder.hessian_keys)

    def add_call(self, tr, xs, seen, oracle_calls, oracle_evals, converged):
        """seen: per iteration dict(d=, lam=, s_norm=, y_norm=) as the callback read them"""
        assert len(tr) == len(xs) == len(seen), (len(tr), len(xs), len(seen))
        its = [dict(tr=dict(r), x=np.array(x, dtype=np.float64), **s) for r, x, s in zip(tr, xs, seen)]
        self.calls.append(dict(its=its, oracle_calls=int(oracle_calls), oracle_evals=int(oracle_evals), converged=bool(converged)))


class Report:
    QUANTITIES = ("d", "z", "gnorm", "f", "trial", "x_next", "sequence", "counts", "decision", "t", "lambda", "s_norm", "y_norm", "stop")

    def __init__(self):
        self.worst = {q: 0.0 for q in self.QUANTITIES}
        self.problems = []
        self.iterations = self.skipped = self.undecidable = 0
        self.branches = {"accept": 0, "halve": 0, "interp": 0, "half_interp": 0, "shrink": 0, "nonfinite": 0, "exhausted": 0}
        self.neg_sy = self.clamp_lo = self.clamp_hi = self.moved = self.not_moved = self.ring_shifts = self.nonmonotone = 0
        self.ring_short = self.ring_long = 0  # decisions, the ring full, that a ring of m - 1 / m + 1 values would have taken the other way
        self.nonmonotone_at = []  # iterations (counted over the calls) with f(x_next) > f(x)
        self.edges = []  # per iteration: entries (on lb pushed out, on lb pushed in, on ub pushed out, on ub pushed in)
        self.first_margin = 0.0  # worst bound / margin over the first decision of each search

    def note(self, q, ratio, where, msg=""):
        ratio = float(ratio)
        if not ratio <= self.worst[q]:
            self.worst[q] = ratio if ratio == ratio else INF
        if not ratio <= 1.0:
            self.problems.append((where, q, ratio, msg))

    def exact(self, q, ok, where, msg=""):
        self.note(q, 0.0 if ok else INF, where, msg)

    def line(self, name):
        w = ", ".join(f"{q} {v:.2e}" for q, v in self.worst.items() if v > 0.0)
        return (f"vec replay {name}: {self.iterations} iterations, skipped {self.skipped}, undecidable {self.undecidable}, branches {self.branches}, "
                f"worst ratios: {w or 'all exact'}")


def _out(lo, hi):
    """float64 ends that enclose a longdouble interval"""
    return float(np.nextafter(np.float64(lo), -INF)), float(np.nextafter(np.float64(hi), INF))


def _in_interval(rep, q, v, lo, hi, where, msg=""):
    """ratio |v - mid| / half-width (a degenerate interval: equality)"""
    if lo == hi:
        rep.exact(q, v == lo, where, f"{msg} {v!r} != {lo!r}")
        return
    mid, hw = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rep.note(q, abs(v - mid) / hw, where, f"{msg} {v!r} outside [{lo!r}, {hi!r}]")


def _t_tmp(t_lo, t_hi, gd_lo, gd_hi, c):
    """the interval of the device's t_tmp over (t, gd), or None where it is not monotone or the denominator's interval holds 0"""
    vals, dens, rels, slopes = [], [], [], []
    for t in (t_lo, t_hi):
        for gd in (gd_lo, gd_hi):
            tl, gl = LD(t), LD(gd)
            den = LD(c) - tl * gl
            dens.append(den)
            slopes.append(2 * LD(c) - tl * gl)
            if den == 0:
                return None
            vals.append(LD(-0.5) * tl * tl * gl / den)
            rels.append(LD(U) * (6 + 2 * abs(tl * gl) / abs(den)))
    if not (min(dens) > 0 or max(dens) < 0) or not (min(slopes) > 0 or max(slopes) < 0):
        return None
    rel = max(rels)
    lo, hi = min(vals), max(vals)
    return _out(lo - abs(lo) * rel, hi + abs(hi) * rel)


def _search(run, rep, where, x, fk, g, d, f_max, it, cursor, alts=()):
    """the line search of one iteration, on intervals.  -> (t interval, trials, the accepted trial's point or None, cursor)"""
    ls, rec, n = run.ls, run.rec, x.size
    ex, mag = cross([g], [d])
    gd_lo, gd_hi = _out(ex[0, 0] - gamma(n) * mag[0, 0], ex[0, 0] + gamma(n) * mag[0, 0])
    t_lo = t_hi = 1.0
    i = trials = 0
    accepted = None
    n_ls = it["tr"]["ls_iters"]
    while i < run.max_ls:
        if cursor >= len(rec.order):
            rep.exact("sequence", False, where, f"trial {trials}: the closure was not called again")
            break
        kq = rec.order[cursor]
        cursor += 1
        trials += 1
        xq, ft = rec.points[kq], rec.seen[kq][0]
        a, b = step(x, t_lo, d), step(x, t_hi, d)
        lo, hi = np.fmin(a, b), np.fmax(a, b)
        if ls["kind"] == "btb":
            lo, hi = project(lo, ls["lo"], ls["hi"]), project(hi, ls["lo"], ls["hi"])
        ok = bool(np.all((xq >= lo) & (xq <= hi)))
        rep.exact("trial", ok, where, f"trial {trials - 1}: the point handed to the closure is outside x + [{t_lo!r}, {t_hi!r}] d")
        if ls["kind"] != "gll" and not math.isfinite(ft):  # `continue` without i += 1
            t_lo, t_hi = t_lo * ls["beta"], t_hi * ls["beta"]
            rep.branches["nonfinite"] += 1
            continue
        if ls["kind"] == "btb":
            e = xq - x
            ee, em = cross([e], [e])
            d2_lo, d2_hi = _out(ee[0, 0] - gamma(n) * em[0, 0], ee[0, 0] + gamma(n) * em[0, 0])
            lhs, rhs = ft - fk, [(-ls["c1"] / t) * v for t in (t_lo, t_hi) for v in (max(d2_lo, 0.0), d2_hi)]
        else:
            lhs = ft - (f_max if ls["kind"] == "gll" else fk)
            rhs = [(ls["c1"] * t) * v for t in (t_lo, t_hi) for v in (gd_lo, gd_hi)]
        sure, maybe = lhs <= min(rhs), lhs <= max(rhs)
        mid, hw = 0.5 * (max(rhs) + min(rhs)), 0.5 * (max(rhs) - min(rhs))
        margin = abs(lhs - mid)
        ratio = hw / margin if margin > 0.0 else INF
        if trials == 1:
            rep.first_margin = max(rep.first_margin, ratio)
        took = trials == n_ls  # what the run did, where the replay cannot tell
        if sure != maybe:
            rep.undecidable += 1
            accept = took and i + 1 <= run.max_ls
        else:
            accept = sure
            rep.worst["decision"] = max(rep.worst["decision"], ratio)
        if sure == maybe:  # would a ring one value shorter / longer have decided otherwise?  (counted only where that, too, is decidable)
            for which, fm in alts:
                a_sure, a_maybe = ft - fm <= min(rhs), ft - fm <= max(rhs)
                if a_sure == a_maybe and a_sure != sure:
                    setattr(rep, which, getattr(rep, which) + 1)
        if accept:
            rep.branches["accept"] += 1
            accepted = xq
            break
        if ls["kind"] != "gll":
            t_lo, t_hi = t_lo * ls["beta"], t_hi * ls["beta"]
            rep.branches["shrink"] += 1
        else:
            small_all, small_any = t_hi <= 0.1, t_lo <= 0.1
            if small_all != small_any:
                rep.undecidable += 1
            if small_all:
                t_lo, t_hi = t_lo * 0.5, t_hi * 0.5
                rep.branches["halve"] += 1
            else:
                tt = _t_tmp(t_lo, t_hi, gd_lo, gd_hi, ft - fk)
                if tt is None:
                    rep.undecidable += 1
                    rep.problems.append((where, "t", INF, "t_tmp: the denominator's interval holds 0"))
                    break
                s_lo, s_hi = ls["sigma2"] * t_lo, ls["sigma2"] * t_hi
                in_all = tt[0] > ls["sigma1"] and tt[1] < s_lo
                in_any = tt[1] > ls["sigma1"] and tt[0] < s_hi
                if in_all != in_any:
                    rep.undecidable += 1
                if in_all:
                    t_lo, t_hi = tt
                    rep.branches["interp"] += 1
                else:
                    t_lo, t_hi = tt[0] * 0.5, tt[1] * 0.5
                    rep.branches["half_interp"] += 1
        i += 1
    if accepted is None:
        rep.branches["exhausted"] += 1
    return (t_lo, t_hi), trials, accepted, cursor


def _z_check(run, rep, where, x, g, h, lam, d_dev):
    """item 9 above n = 5: the one norm-wise check"""
    import newton_solve_cases as NS
    n = x.size
    hs = np.tril(h) + np.tril(h, -1).T
    hl = hs.astype(LD)
    z = np.linalg.solve(hs, g).astype(LD)
    inv = np.linalg.inv(hs)
    for _ in range(6):  # refinement with longdouble residuals, LAPACK's inverse as the preconditioner (as newton_solve_cases.solve_extended)
        z = z + (inv @ (g.astype(LD) - hl @ z).astype(np.float64)).astype(LD)
    xi = inv.astype(LD)
    for _ in range(3):  # ||H^-1||_2 of an inverse formed in longdouble (Newton-Schulz from LAPACK's), its norm by a float64 SVD
        xi = xi @ (2 * np.eye(n, dtype=LD) - hl @ xi)
    hinv2 = float(np.linalg.norm(xi.astype(np.float64), 2)) * (1.0 + 1e-6)
    r2 = math.sqrt(n) * NS.bound(n) * (NS.norm_inf(hs) * float(np.max(np.abs(z))) * (1.0 + 1e-3) + float(np.max(np.abs(g))))
    lm = 1.0 if lam is None else lam
    xl = x.astype(LD)
    dz = np.minimum(np.maximum(xl - LD(lm) * z, run.lb), run.ub) - xl
    err = float(np.sqrt(np.sum((d_dev.astype(LD) - dz) ** 2)))
    bound = lm * hinv2 * r2 + 4 * U * (float(np.linalg.norm(x)) + lm * float(np.sqrt(np.sum(z * z))))
    rep.note("z", err / bound if bound > 0.0 else (0.0 if err == 0.0 else INF), where, f"||d - d(z*)||_2 = {err:.3e} against {bound:.3e}")


def replay(run):
    rep, rec, n = Report(), run.rec, run.x0.size
    lb, ub, ls = run.lb, run.ub, run.ls
    spectral, needs_y, newton = run.method in ("spg", "spn"), run.method != "pgd", run.method in ("pn", "spn")
    full = not run.limited
    x, lam, cursor = run.x0, None, 0
    if spectral:  # the constructor's evaluation: lambda0 = clamp(1 / ||P(x0 - g0) - x0||_inf)
        if full:
            rep.exact("sequence", bool(rec.order) and rec.order[0] == key(x), "constructor", "the first evaluation is not at P(x0)")
            cursor = 1
            g0 = rec.grad(x, "x_0")
        else:
            g0 = run.grads[0]
        with np.errstate(divide="ignore"):
            dm = np.float64(np.fmax.reduce(np.abs(direction(x, g0, None, lb, ub)), initial=0.0))
            lam = clamp(np.float64(1.0) / dm, *run.ctor_lams)  # (with_lambdas acts from the first update on: the constructor clamps with its defaults)
        rep.exact("lambda", lam == run.lam0, "constructor", f"lambda0 {run.lam0!r} against {lam!r}")
        lam = run.lam0
    ring, hist, s_prev, y_prev, gi, xks = [], [], None, None, 0, []
    for ci, call in enumerate(run.calls):
        held = None  # a host closure's evaluation is not kept from one call to the next
        real, ncalls = 0, 0
        for k, it in enumerate(call["its"]):
            where, tr = (ci, k), it["tr"]
            rep.iterations += 1
            if full:
                kx = key(x)
                if not (run.memoize and held == kx):
                    ok = cursor < len(rec.order) and rec.order[cursor] == kx
                    rep.exact("sequence", ok, where, "the loop top's evaluation is not at x_k")
                    cursor += 1
                    real += 1
                if kx not in rec.seen:
                    rep.exact("sequence", False, where, "x_k was never evaluated")
                    return rep
                fk, g = rec.seen[kx]
                rep.exact("f", tr["f"] == fk, where, f"trace f {tr['f']!r} against the closure's {fk!r}")
            else:
                g = run.grads[gi]
            pg = pg_norm(x, g, lb, ub)
            rep.exact("gnorm", tr["gnorm"] == pg, where, f"trace gnorm {tr['gnorm']!r} against {pg!r}")
            rep.exact("stop", not pg < run.tol, where, "the run went on although ||pg||_inf < tol")
            rep.edges.append((int(np.sum((x == lb) & (g > 0))), int(np.sum((x == lb) & (g < 0))), int(np.sum((x == ub) & (g < 0))), int(np.sum((x == ub) & (g > 0)))))
            if run.method == "pn" and s_prev is not None:
                rep.exact("stop", not s_prev < run.tol and not y_prev < run.tol, where, "the run went on although s_norm or y_norm < tol")
            # ---- the direction ----
            d = it["d"]
            w = g
            if newton:
                xks.append(key(x))
                h = rec.hess[key(x)]
                if n <= SMALL_N:
                    w = small_solve(h, g)
                else:
                    w = None
                    _z_check(run, rep, where, x, g, h, lam if spectral else None, d)
            if w is not None:
                dk = direction(x, w, lam if spectral else None, lb, ub)
                rep.exact("d", same(d, dk), where, f"direction differs at entry {first_diff(d, dk)}")
            t = tr["t"]
            xn = step(x, t, d)
            rep.exact("x_next", same(it["x"], xn), where, f"x_next is not x + t d at entry {first_diff(it['x'], xn)}")
            evaluated = True
            if full:
                # ---- the line search ----
                f_max, alts = None, []
                if ls["kind"] == "gll":
                    if len(ring) == ls["m"]:
                        ring.pop(0)
                        rep.ring_shifts += 1
                    ring.append(fk)
                    hist.append(fk)
                    f_max = float(np.fmax.reduce(np.array(ring), initial=-INF))
                    if len(hist) > ls["m"]:  # the ring is full and has shifted
                        if ls["m"] > 1:
                            alts.append(("ring_short", float(np.fmax.reduce(np.array(hist[-(ls["m"] - 1):])))))
                        alts.append(("ring_long", float(np.fmax.reduce(np.array(hist[-(ls["m"] + 1):])))))
                (t_lo, t_hi), trials, acc, cursor = _search(run, rep, where, x, fk, g, d, f_max, it, cursor, alts)
                real += trials
                if t_hi - t_lo > CAP * abs(t):
                    rep.skipped += 1
                else:
                    _in_interval(rep, "t", t, t_lo, t_hi, where, "trace t")
                rep.exact("counts", tr["ls_iters"] == trials, where, f"ls_iters {tr['ls_iters']} against {trials} trials replayed")
                rep.exact("counts", tr["n_evals"] == 1 + trials + (1 if needs_y else 0), where, f"n_evals {tr['n_evals']} with {trials} trials")
                ncalls += 1 + trials + (1 if needs_y else 0)
                evaluated = acc is not None
                if acc is not None:
                    want = project(xn, ls["lo"], ls["hi"]) if ls["kind"] == "btb" else xn
                    rep.exact("trial", same(acc, want), where, f"the accepted trial is not (the projection of) x + t d at entry {first_diff(acc, want)}")
                    if ls["kind"] == "btb":
                        moved = not same(acc, xn)
                        evaluated = not moved
                        rep.moved += 1 if moved else 0
                        rep.not_moved += 0 if moved else 1
                # ---- the evaluation at x_next ----
                kn = key(xn)
                if needs_y:
                    if not (run.memoize and evaluated):
                        ok = cursor < len(rec.order) and rec.order[cursor] == kn
                        rep.exact("sequence", ok, where, "no evaluation at x_next = x + t d behind the search")
                        cursor += 1
                        real += 1
                    held = kn
                else:
                    held = kn if (run.memoize and evaluated) else None
                if kn in rec.seen and rec.seen[kn][0] > fk:
                    rep.nonmonotone += 1
                    rep.nonmonotone_at.append(rep.iterations - 1)
            # ---- the update scalars ----
            s = xn - x
            if needs_y:
                if full:
                    if key(xn) not in rec.seen:
                        rep.exact("sequence", False, where, "x_next was never evaluated")
                        return rep
                    gn = rec.seen[key(xn)][1]
                else:
                    gn = run.grads[gi + 1]
                y = gn - g
                ex, mag = cross([s, y], [s, y])
                ss, sy, yy = ex[0, 0], ex[0, 1], ex[1, 1]
                bss, bsy = gamma(n) * mag[0, 0], gamma(n) * mag[0, 1]
                rs = float(0.5 * gamma(n) + 2 * U) * 1.001  # sqrt halves the sum's relative bound; its own rounding, and the bound's evaluation
                sn = float(np.sqrt(ss))
                _in_interval(rep, "s_norm", tr["s_norm"], sn * (1 - rs), sn * (1 + rs), where, "trace s_norm")
                if run.method == "pn":
                    yn = float(np.sqrt(yy))
                    _in_interval(rep, "y_norm", tr["y_norm"], yn * (1 - rs), yn * (1 + rs), where, "trace y_norm")
                    rep.exact("s_norm", it["s_norm"] == tr["s_norm"], where, "s_norm() is not the trace's")
                    rep.exact("y_norm", it["y_norm"] == tr["y_norm"], where, "y_norm() is not the trace's")
                    s_prev, y_prev = it["s_norm"], it["y_norm"]
                if spectral:
                    lam_dev = it["lam"]
                    if not abs(sy) > bsy:
                        rep.undecidable += 1
                    elif sy < 0:
                        rep.neg_sy += 1
                        rep.exact("lambda", lam_dev == run.lam_max, where, f"s.y = {float(sy):.3e} <= 0 but lambda = {lam_dev!r}")
                    else:
                        q = ss / sy
                        ry = bsy / abs(sy)
                        r = (bss / ss + ry) / (1 - ry) + LD(2 * U)
                        q_lo, q_hi = _out(q * (1 - r), q * (1 + r))
                        l_lo, l_hi = clamp(q_lo, run.lam_min, run.lam_max), clamp(q_hi, run.lam_min, run.lam_max)
                        rep.clamp_lo += 1 if l_hi == run.lam_min else 0
                        rep.clamp_hi += 1 if l_lo == run.lam_max else 0
                        if l_hi - l_lo > CAP * l_lo:
                            rep.skipped += 1
                        else:
                            _in_interval(rep, "lambda", lam_dev, l_lo, l_hi, where, "lambda")
                    lam = lam_dev
            else:
                rep.exact("s_norm", tr["s_norm"] == 0.0, where, "projected gradient keeps no s_norm")
            x = xn
            gi += 1
        if full:
            if call["converged"]:  # the run ended at a loop top: its evaluation, then the stop rule in its order
                kx = key(x)
                if not (run.memoize and held == kx):
                    ok = cursor < len(rec.order) and rec.order[cursor] == kx
                    rep.exact("sequence", ok, (ci, "end"), "the last loop top's evaluation is not at x")
                    cursor += 1
                    real += 1
                ncalls += 1
                if kx in rec.seen:
                    stop = pg_norm(x, rec.seen[kx][1], lb, ub) < run.tol
                    if run.method == "pn" and s_prev is not None:
                        stop = stop or s_prev < run.tol or y_prev < run.tol
                    rep.exact("stop", stop, (ci, "end"), "the run ended although no stop rule holds")
            rep.exact("counts", call["oracle_calls"] == ncalls, (ci, "end"), f"oracle_calls {call['oracle_calls']} against {ncalls}")
            rep.exact("counts", call["oracle_evals"] == real, (ci, "end"), f"oracle_evals {call['oracle_evals']} against {real}")
    if full and newton and run.hessian_calls:
        rep.exact("sequence", rec.hessian_keys == xks, "end", f"{len(rec.hessian_keys)} Hessian callbacks against {len(xks)} iterations, or not at x_k")
    if full:
        rep.exact("sequence", cursor == len(rec.order), "end", f"{len(rec.order) - cursor} evaluations the replay does not account for")
    return rep


def check(rep, name):
    """the assertion of both tests: every ratio at most 1, every equality exact, nothing skipped, nothing undecidable"""
    print(rep.line(name))
    assert not rep.problems, (name, rep.problems[:4])
    assert rep.skipped == 0 and rep.undecidable == 0, (name, rep.skipped, rep.undecidable)
    assert all(v <= 1.0 for v in rep.worst.values()), (name, rep.worst)
