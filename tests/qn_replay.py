"""The replay of a dense quasi-Newton run (DFP, BFGS, SR1, Broyden; free or in a box) from its own recorded iterates in extended precision: what
tests/lse_eval_cases.py (the log-sum-exp objective), tests/quad_replay_cases.py (device quadratics) and tests/broyden_replay_cases.py share.  Test infrastructure: the product does
not import this file.

A TRUTH is any object with f, g (np.longdouble) at a point and the bounds bf, bg (float64) a float64 evaluation of that objective must meet, plus
gnorm = ||g|| and bgnorm = ||bg||; the replay is given a factory x -> truth.  tests/lse_eval_cases.py's docstring says which point a trace field
belongs to and derives every half-width below; what this file adds to it:

  A START MATRIX.  InverseHessian(n, method, h0): h0 is a float64 matrix read back from the device and TAKEN AS EXACT (the next call of the solver
  starts from those very bits), so H_k = h0 + the replayed terms, Habs starts at |h0| and DH at 0.  A run is then replayed in short segments that
  restart from the H just read, and the bound on the device's H -- which loses a factor of 5-8 per replayed iteration -- never accumulates further
  than a segment is long.

  SR1 (sr1_b.rs:144-146).  u = H y, c = 1 / (s'y - y'u), H+ = H + c (s s' - s u' - u s' + u u'): the three-coefficient form with c_ss = c_uu = c,
  c_su = -c.  The denominator, whether the device forms it as s'y - y'u or as (s - u)'y, is off by at most dys + dyu (the two inner products' own
  bounds, each a sum of magnitudes) plus the subtraction's rounding, hence c by _inv_bound(s'y - y'u, dys + dyu + 2 eps |s'y - y'u|).  An update
  that cannot be bounded makes the later direction checks and the H check `skipped`.

  BROYDEN (broyden.rs:115-118).  u = H y, a = s - u, w = H' s (a row vector times H: the COLUMN sums), c = 1 / s'y -- the denominator as the
  reference writes it, not s'Hy -- and H+ = H + c a w': one term (c, a, w), not symmetric, so `times_t` forms H' v (h0' in row chunks plus the
  terms with p and q exchanged).  s = fl(x+ - x) is the device's own, bit for bit.  With the device's H off by at most DH entry by entry:
      du   as for the other methods;
      dw = DH' |s| + (n + 4) eps Habs' |s|            (a column sum of n products, bracketed anyhow: per-lane chains, four waves, the tile rows);
      da = du + eps (|s| + |u| + du)                  (one subtraction of the computed u);
      dc = _inv_bound(s'y, dys)                       (dys the inner product's own bound, as for DFP's 1 / s'y).
  Habs grows by |c| |a| |w|', and every factor of c a w' moved by its bound, written out as non-negative terms:
      DH+ = DH + dc (|a| + da)(|w| + dw)' + |c| (da |w|' + |a| dw' + da dw') + 8 eps Habs+.
  The applied update h + c (a_i w_j) is three roundings, each of a quantity Habs+ bounds: 3 eps Habs+ at first order, inside the 8.
  THE LAZY DIRECTION (qn_ctl_step.hip.h, QN_ST_AFTER_U) is another bracketing of H+ g+: d+ = -(v + c (a (w . g+))) with v = H g+ from the
  same pass.  v is held by the row sum's bound with |H| and DH; w . g+ is off by (|w| + dw) . bg + dw . |g| + (n + 2) eps (|w| + dw) . (|g| + bg);
  c, a move by dc, da; three products and one addition round once each.  Collected:
      |d+ + H+ g+| <= Habs+ bg + (n + 4) eps Habs+ |g| + [DH + dc (..)(..)' + |c| (..)] (|g| + bg) + 4 eps Habs+ |g|,
  which is `apply`'s bound with DH+ (the bracket is DH+ less its 8 eps Habs+, of which the four roundings take half) PROVIDED the sum's term
  (n + 4) eps |H| |g| is taken with Habs+ = |H| + |c| |a| |w|' in the place of |H+|: the magnitudes of the two addends, which cancellation
  between H and c a w' can leave far above |H + c a w'|.  The dense |H+| the other methods use does not cover that, so for this method
  `apply` takes Habs (>= |H_k| entry by entry, and what either bracketing sums in magnitude).  `symmetric` is never set for it; the caller
  asserts instead that the matrix read back is clearly NOT symmetric, max |H - H'| far above `Report.dh_max` = max DH.

  A BOX (bfgs_b.rs compute_direction / update_next_iterate).  d = P(x - H g) - x and x+ = x + t d.  Projection onto a box is 1-Lipschitz entry by
  entry, so entry j of x_{k+1} - x_k is held to t (clip(x_j - (H_k g_k)_j, lb_j, ub_j) - x_j) with the half-width of the free step plus
  2 eps t (|lb_j| + |ub_j|) on finite bounds (the bound itself rounded into the difference, and a trial point clamped again).  No entry is classified.

  THE CHECK `H`.  Given the matrix approx_inv_hessian() returns at the end of a segment of K iterations: entry by entry
      |H_dev - H_K| <= DH_K + 8 eps Habs_K,
  H_K formed densely in longdouble from h0 and the segment's terms; and H_dev == H_dev' bit for bit where the path promises it (`symmetric`).  With
  max DH_K > CAP max |H_K| the check proves nothing and is skipped, not asserted (it counts in the skip cap).

Every check is a ratio |error| / bound; the assertion is ratio <= 1 (`check`).  `Tally` holds the skip caps: at most SKIP_SHARE of the (run, iteration,
check) triples skipped, iteration 0 of every replayed segment asserted (its f, gnorm, s_norm, y_norm and dir; the H check of a one-iteration
segment is under the next rule alone), no segment with every direction check skipped, and (add_run) no run with every H check skipped."""
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
INF = float("inf")
REPLAY = 3           # iterations of a run (or segment) whose direction is replayed
CAP = 1e-6           # discrimination of the direction check and of the H check
Y_CAP = 1e-3         # ... and of y_norm
SKIP_SHARE = 0.10
CHECKS = ("f", "gnorm", "s_norm", "y_norm", "dir")
ROWS = 256           # longdouble products of a float64 matrix go in row chunks: no longdouble copy of the matrix


def ld_matvec(mat, v):
    """mat @ v in longdouble, mat float64 (n x n), chunk by chunk"""
    vl = v.astype(LD)
    out = np.empty(mat.shape[0], dtype=LD)
    for i in range(0, mat.shape[0], ROWS):
        out[i:i + ROWS] = mat[i:i + ROWS].astype(LD) @ vl
    return out


def coefficients(method, ys, yu):
    """(c_ss, c_su, c_uu) of H+ = H + c_ss s s' + c_su (s u' + u s') + c_uu u u'"""
    if method == "bfgs":
        return (1 + yu / ys) / ys, -1 / ys, 0 * ys
    if method == "sr1":
        c = 1 / (ys - yu)
        return c, -c, c
    return 1 / ys, 0 * ys, -1 / yu


def _ratio(err, bound):
    """max |err| / bound; anything not finite, or an error against a zero bound, is inf"""
    err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound))):
        return INF
    with np.errstate(all="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, INF))
    return float(np.max(r))


def point_ratios(tr, f, g):
    """(ratio of f, ratio of g entry by entry) of an evaluation against the truth `tr` at the same point"""
    return _ratio(float(abs(LD(f) - tr.f)), tr.bf), _ratio((np.asarray(g, dtype=np.float64).astype(LD) - tr.g).astype(np.float64), tr.bg)


class Report:
    def __init__(self, name, kind="lse"):
        self.name, self.kind = name, kind
        self.rows = []  # (iteration, check, ratio, asserted)
        self.dh_max = None  # max DH at the segment's end, where the H check ran

    def add(self, k, check, ratio, asserted=True):
        self.rows.append((k, check, float(ratio), bool(asserted)))

    @property
    def worst(self):
        return max([r for _, _, r, a in self.rows if a] + [0.0])

    def worst_of(self, check):
        return max([r for _, c, r, a in self.rows if a and c == check] + [0.0])

    @property
    def skipped(self):
        return [(k, c) for k, c, _, a in self.rows if not a]

    def line(self):
        checks = CHECKS + (("H",) if any(c == "H" for _, c, _, _ in self.rows) else ())
        per = ", ".join(f"{c} {self.worst_of(c):.2e}" for c in checks)
        return f"{self.kind} replay {self.name}: worst {self.worst:.3e} ({per}), checks {len(self.rows)}, skipped {self.skipped}"


def _inv_bound(v, dv):
    """bound on |1 / v^ - 1 / v| for |v^ - v| <= dv, plus the division's own rounding"""
    v = abs(float(v))
    if not dv < v:
        return INF
    return dv / (v * (v - dv)) + 2.0 * EPS / (v - dv)


def _outer(u, v):
    return np.multiply.outer(u, v)


class InverseHessian:
    """H_k in longdouble from the replayed pairs, kept as H = H_0 + sum coef p q' with H_0 = I or the float64 start matrix h0 (products H v cost
    O(n k) longdouble operations on top of h0 v; |H_k| is formed densely in float64, where it only scales a bound), Habs >= |H_k| and
    DH >= |H_k of the device - H_k| in float64 (tests/lse_eval_cases.py's docstring, `dir`)"""

    def __init__(self, n, method, h0=None):
        self.n, self.method, self.terms, self.habs, self.dh, self.bounded = n, method, [], None, None, True
        self.h0 = None if h0 is None else np.ascontiguousarray(h0, dtype=np.float64)
        if self.h0 is not None:
            assert self.h0.shape == (n, n)
            self.habs, self.dh = np.abs(self.h0), np.zeros((n, n))

    def times(self, v):
        out = v.astype(LD) if self.h0 is None else ld_matvec(self.h0, v)
        for coef, p, q in self.terms:
            out = out + (coef * np.dot(q, v)) * p
        return out

    def times_t(self, v):
        """H_k' v: h0' in row chunks (row i of h0 scaled by v_i, summed over the chunk), plus the terms with p and q exchanged"""
        vl = v.astype(LD)
        if self.h0 is None:
            out = vl.copy()
        else:
            out = np.zeros(self.n, dtype=LD)
            for i in range(0, self.n, ROWS):
                out = out + vl[i:i + ROWS] @ self.h0[i:i + ROWS].astype(LD)
        for coef, p, q in self.terms:
            out = out + (coef * np.dot(p, vl)) * q
        return out

    def dense_abs(self):
        h = np.eye(self.n) if self.h0 is None else self.h0.copy()
        for coef, p, q in self.terms:
            h += float(coef) * _outer(p.astype(np.float64), q.astype(np.float64))
        return np.abs(h) * (1.0 + 1e-9)

    def dense_rows(self, lo, hi):
        """rows [lo, hi) of H_k, longdouble"""
        h = np.zeros((hi - lo, self.n), dtype=LD)
        if self.h0 is None:
            h[np.arange(hi - lo), np.arange(lo, hi)] = 1
        else:
            h += self.h0[lo:hi]
        for coef, p, q in self.terms:
            h += _outer(coef * p[lo:hi], q)
        return h

    def apply(self, g, gabs, bg):
        """(H g, |H| bg + (n + 4) eps |H| |g| + DH (|g| + bg))"""
        if not self.terms and self.h0 is None:
            return g, bg + (self.n + 4) * EPS * gabs
        if not self.bounded:
            return self.times(g), np.full(self.n, INF)
        habs = self.habs if self.method == "broyden" else self.dense_abs()  # (Broyden: the lazy direction sums |H| + |c| |a| |w|', the docstring)
        return self.times(g), (habs @ bg + (self.n + 4) * EPS * (habs @ gabs) + self.dh @ (gabs + bg)) * (1.0 + 1e-9)

    def update(self, s, y, dy):
        n = self.n
        if self.habs is None:
            self.habs, self.dh = np.eye(n), np.zeros((n, n))
        sl, sa, ya = s.astype(LD), np.abs(s), np.abs(y).astype(np.float64)
        u = self.times(y)
        ua = np.abs(u).astype(np.float64)
        if self.method == "broyden":
            return self._update_broyden(sl, sa, y, ya, dy, u, ua)
        ys, yu = np.dot(sl, y), np.dot(y, u)
        css, csu, cuu = coefficients(self.method, ys, yu)
        if self.method == "bfgs":
            self.terms += [(css, sl, sl), (csu, sl, u), (csu, u, sl)]
        elif self.method == "sr1":
            self.terms += [(css, sl, sl), (csu, sl, u), (csu, u, sl), (cuu, u, u)]
        else:
            self.terms += [(css, sl, sl), (cuu, u, u)]
        du = self.dh @ ya + self.habs @ dy + (n + 4) * EPS * (self.habs @ (ya + dy))
        ub = ua + du
        dys = float(sa @ dy) + (n + 2) * EPS * float(sa @ (ya + dy))
        dyu = float(dy @ ub) + float(ya @ du) + (n + 2) * EPS * float((ya + dy) @ ub)
        ys, yu = float(ys), float(yu)
        d_iys = _inv_bound(ys, dys)
        if self.method == "bfgs":
            acss, acsu, acuu = abs(float(css)), abs(float(csu)), 0.0
            dcsu, dcuu = d_iys, 0.0
            dcss = d_iys + ((abs(yu) + dyu) / (abs(ys) - dys) ** 2 - abs(yu) / ys ** 2 if dys < abs(ys) else INF) + 4.0 * EPS * acss
        elif self.method == "sr1":
            acss = acsu = acuu = abs(float(css))
            dcss = dcsu = dcuu = _inv_bound(ys - yu, dys + dyu + 2.0 * EPS * abs(ys - yu))
        else:
            acss, acsu, acuu = abs(float(css)), 0.0, abs(float(cuu))
            dcss, dcsu, dcuu = d_iys, 0.0, _inv_bound(yu, dyu)
        if not all(math.isfinite(v) for v in (dcss, dcsu, dcuu)) or not np.all(np.isfinite(du)):
            self.bounded = False
            return
        if self.method == "bfgs":
            self.habs += acss * _outer(sa, sa) + acsu * (_outer(sa, ua) + _outer(ua, sa))
            dt = dcss * _outer(sa, sa) + acsu * (_outer(sa, du) + _outer(du, sa)) + dcsu * (_outer(sa, ub) + _outer(ub, sa))
        elif self.method == "sr1":
            self.habs += acss * (_outer(sa, sa) + _outer(sa, ua) + _outer(ua, sa) + _outer(ua, ua))
            dt = (dcss * (_outer(sa, sa) + _outer(sa, ub) + _outer(ub, sa) + _outer(ub, ub))
                  + acss * (_outer(sa, du) + _outer(du, sa) + _outer(ua, du) + _outer(du, ua) + _outer(du, du)))
        else:
            self.habs += acss * _outer(sa, sa) + acuu * _outer(ua, ua)
            dt = dcss * _outer(sa, sa) + acuu * (_outer(ua, du) + _outer(du, ua) + _outer(du, du)) + dcuu * _outer(ub, ub)
        self.dh = (self.dh + dt + 8.0 * EPS * self.habs) * (1.0 + 1e-9)

    def _update_broyden(self, sl, sa, y, ya, dy, u, ua):
        """H+ = H + c a w', a = s - u, w = H' s, c = 1 / s'y (the docstring's paragraph BROYDEN)"""
        n = self.n
        w = self.times_t(sl)
        a = sl - u
        ys = np.dot(sl, y)
        with np.errstate(divide="ignore"):  # (s'y = 0: dc below is not finite and the update counts as not bounded)
            c = 1 / ys
        self.terms.append((c, a, w))
        aa, wa, ac = np.abs(a).astype(np.float64), np.abs(w).astype(np.float64), abs(float(c))
        du = self.dh @ ya + self.habs @ dy + (n + 4) * EPS * (self.habs @ (ya + dy))
        dw = self.dh.T @ sa + (n + 4) * EPS * (self.habs.T @ sa)
        da = du + EPS * (sa + ua + du)
        dys = float(sa @ dy) + (n + 2) * EPS * float(sa @ (ya + dy))
        dc = _inv_bound(float(ys), dys)
        if not math.isfinite(dc) or not np.all(np.isfinite(du)) or not np.all(np.isfinite(dw)):
            self.bounded = False
            return
        self.habs += ac * _outer(aa, wa)
        dt = dc * _outer(aa + da, wa + dw) + ac * (_outer(da, wa) + _outer(aa, dw) + _outer(da, dw))
        self.dh = (self.dh + dt + 8.0 * EPS * self.habs) * (1.0 + 1e-9)

    def check_dense(self, h_dev):
        """(ratio, assertable) of the stored matrix against H_k: |H_dev - H_k| <= DH + 8 eps Habs entry by entry"""
        n = self.n
        h_dev = np.asarray(h_dev, dtype=np.float64)
        if h_dev.shape != (n, n) or not np.all(np.isfinite(h_dev)):
            return INF, True
        if not self.bounded:
            return INF, False
        if self.habs is None:  # no update at all: H_0 = I (or h0) as it is
            habs, dh = (np.eye(n) if self.h0 is None else np.abs(self.h0)), np.zeros((n, n))
        else:
            habs, dh = self.habs, self.dh
        worst, hmax = 0.0, 0.0
        for lo in range(0, n, ROWS):
            hi = min(n, lo + ROWS)
            hk = self.dense_rows(lo, hi)
            hmax = max(hmax, float(np.max(np.abs(hk))))
            worst = max(worst, _ratio((h_dev[lo:hi].astype(LD) - hk).astype(np.float64), dh[lo:hi] + 8.0 * EPS * habs[lo:hi]))
        return worst, float(np.max(dh)) <= CAP * hmax


def replay(name, truth, x0, method, tr, xs, h0=None, box=None, h_dev=None, symmetric=False, iters=REPLAY, kind="qn"):
    """Report of a run or of one segment of it.  truth: x -> truth object; tr the trace records (f, gnorm, t, s_norm, y_norm, updated) of the
    segment, xs[k] = x_{k+1}, x0 the point it starts from, h0 the matrix it starts from (None: I); box = (lb, ub) of a bounded solver; h_dev the
    matrix read at the segment's end (None: no H check; only with len(tr) <= iters), symmetric: whether it must equal its transpose bit for bit."""
    x = np.array(x0, dtype=np.float64)
    n = x.size
    rep = Report(name, kind)
    assert len(tr) >= 1 and len(xs) >= len(tr), (len(tr), len(xs))
    iters = min(len(tr), iters)
    want_h = h_dev is not None
    assert not want_h or iters == len(tr), "the H check needs every iteration of the segment replayed"
    hk = InverseHessian(n, method, h0)
    finite = None if box is None else (np.where(np.isfinite(box[0]), np.abs(box[0]), 0.0) + np.where(np.isfinite(box[1]), np.abs(box[1]), 0.0))
    for k in range(iters):
        r, xn = tr[k], np.array(xs[k], dtype=np.float64)
        if not np.all(np.isfinite(xn)):
            rep.add(k, "dir", INF)
            break
        t0, t1 = truth(x), truth(xn)
        rep.add(k, "f", _ratio(float(abs(LD(r["f"]) - t0.f)), t0.bf))
        gsum = ((n + 2) * EPS + EPS) * (t0.gnorm + t0.bgnorm)
        rep.add(k, "gnorm", _ratio(r["gnorm"] - t0.gnorm, t0.bgnorm + gsum))
        s = xn - x
        sl = s.astype(LD)
        snorm = float(np.sqrt(np.dot(sl, sl)))
        rep.add(k, "s_norm", _ratio(r["s_norm"] - snorm, ((n + 2) * EPS + EPS) * snorm))
        y = t1.g - t0.g
        dy = t1.bg + t0.bg + EPS * np.abs(y).astype(np.float64)
        ynorm, dynorm = float(np.sqrt(np.dot(y, y))), float(np.linalg.norm(dy))
        rep.add(k, "y_norm", _ratio(r["y_norm"] - ynorm, dynorm + ((n + 3) * EPS) * (ynorm + dynorm)), asserted=dynorm <= Y_CAP * ynorm)
        t = float(r["t"])
        gabs = np.abs(t0.g).astype(np.float64)
        hg, spread = hk.apply(t0.g, gabs, t0.bg)
        hw = t * spread + 2.0 * EPS * (np.abs(x) + np.abs(xn))
        if box is None:
            step = -LD(t) * hg
        else:
            step = LD(t) * (np.clip(x.astype(LD) - hg, box[0].astype(LD), box[1].astype(LD)) - x.astype(LD))
            hw = hw + 2.0 * EPS * t * finite
        hw = hw * (1.0 + 1e-9)
        smax = float(np.max(np.abs(s)))
        bounded = bool(np.all(np.isfinite(hw)))
        ratio = _ratio((sl - step).astype(np.float64), hw) if bounded else INF
        rep.add(k, "dir", ratio, asserted=bounded and float(np.max(hw)) <= CAP * smax)
        if (k + 1 < iters or want_h) and r["updated"]:
            hk.update(s, y, dy)
        x = xn
    if want_h:
        ratio, ok = hk.check_dense(h_dev)
        if symmetric and not np.array_equal(h_dev, np.asarray(h_dev).T):
            ratio, ok = INF, True
        rep.add(iters - 1, "H", ratio, asserted=ok)
        rep.dh_max = float(np.max(hk.dh)) if hk.dh is not None and hk.bounded else (0.0 if hk.bounded else INF)
    return rep


class Tally:
    """the skip caps over everything that was replayed"""

    def __init__(self):
        self.triples = self.skipped = 0

    def add(self, rep):
        """per run or segment: iteration 0 asserted, not every direction check skipped.  (The H check carries the index of the segment's last
        iteration and has its own cap, add_run's: in a segment of ONE iteration it sits at index 0 and may still be skipped -- the rule about
        iteration 0 is about f, gnorm, s_norm, y_norm and dir, which at iteration 0 of a segment depend on no replayed update.)"""
        self.triples += len(rep.rows)
        self.skipped += len(rep.skipped)
        assert not [kc for kc in rep.skipped if kc[0] == 0 and kc[1] != "H"], (rep.name, "iteration 0 must be asserted", rep.skipped)
        assert any(a for _, c, _, a in rep.rows if c == "dir"), (rep.name, "every direction check skipped")

    def add_run(self, reps):
        """the segments of one run: each as `add`, and not every H check of the run skipped"""
        for rep in reps:
            self.add(rep)
        hs = [a for rep in reps for _, c, _, a in rep.rows if c == "H"]
        assert not hs or any(hs), ([rep.name for rep in reps], "every H check skipped")

    def check(self):
        assert self.skipped <= SKIP_SHARE * self.triples, (self.skipped, self.triples)


def check(rep):
    print(rep.line())
    bad = [(k, c, r) for k, c, r, a in rep.rows if a and not r <= 1.0]
    assert not bad, (rep.name, bad[:6])
