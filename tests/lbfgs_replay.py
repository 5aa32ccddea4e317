"""Replay of an L-BFGS run, iteration by iteration, in extended precision from the run's own pairs (tests/test_ref_lbfgs_replay.py licenses it on
the float64 restatement, tests/test_gpu_lbfgs_replay.py applies it to the GPU).  Test infrastructure: the product does not import this file.

A run on a host closure can be rebuilt from the outside.  The solver receives g from the closure bit for bit, forms s = x_next - x and
y = g_next - g with one subtraction each, and the step as u = x - z, d = min(max(u, lb), ub) - x, x_next = x + t d.  The trace keeps every x_k and
t_k.  So every iteration is checked ON ITS OWN: the memory is rebuilt from the run's iterates (`updated[k]` and a rise of `resets()` are taken as
given), z = H_k g_k is evaluated in numpy.longdouble by the TWO-LOOP recursion -- not the compact form the kernels use -- x_{k+1} is predicted
and compared element by element.  Nothing accumulates from one iteration to the next.

HOW z IS EVALUATED.  Every vector of the two-loop recursion lies in span(g, Y, S), so the recursion is run on coefficients: its inner products
s_i.q and y_i.r are expanded through the longdouble sums S'g, Y'g, S'Y, Y'Y (each formed once, chunk by chunk, from the float64 pairs), and
z = gamma g + sum_j (a_j y_j + b_j s_j) is then formed element by element in longdouble.  That is the recursion statement by statement (alpha_i,
q -= alpha_i y_i, r = gamma q, beta_i, r += (alpha_i - beta_i) s_i), with no triangular solve in it, and costs two passes over the memory
whatever n is (the n = 2^21 + 2 case replays in seconds, with no temporary longer than a chunk).

THE BOUND dz on |computed z - exact z|, element by element.  It holds for the compact form
    w = R^-1 p,  u = R^-T [(D + gamma Y'Y) w - gamma q],  z = gamma g + S u - gamma Y w,     R = triu(S'Y), D = diag(R), p = S'g, q = Y'g
evaluated in float64 in ANY summation order, with or without fused multiply-adds.  eps = 2^-52 throughout, twice the unit roundoff: the
factor of two pays for the second-order terms and for evaluating the bound itself in floating point (sums of non-negative terms only).
  1. A sum of n products carries at most (n + 2) eps times the sum of their magnitudes, in any order:
         dp_i = g_n |S_i|.|g|,  dq_i = g_n |Y_i|.|g|,  ER_ij = g_n |S_i|.|y_j|,  EW_ij = g_n |Y_i|.|Y_j|,      g_n = (n + 2) eps.
  2. A triangular solve of order k by substitution, any order, solves a system with the matrix perturbed by at most g_k |R^| element-wise (Higham,
     Accuracy and Stability, thm 8.5; g_k = (k + 2) eps).  With E = ER + g_k (|R| + ER) the computed w^ satisfies
         |w^ - w| <= |R^-1| (dp + E |w^|),   |w^| <= |w| + dw   ==>   dw = (I - |R^-1| E)^-1 |R^-1| (dp + E |w|),
     valid when that solution exists, is non-negative and satisfies its own inequality; otherwise dw = inf (the iteration proves nothing).
  3. gamma = s_p.y_p / y_p.y_p: the numerator's relative error is g_n |s_p|.|y_p| / s_p.y_p, the denominator's g_n (all terms positive), the
     division adds eps:  dgamma = gamma r / (1 - r),  r = g_n (|s_p|.|y_p| / s_p.y_p + 1) + eps.  Unit scaling: gamma = 1, dgamma = 0.
  4. The middle vector rr = (D + gamma Y'Y) w - gamma q: every product of perturbed factors satisfies |a^ b^ - a b| <= (|a| + da)(|b| + db) - |a| |b|,
     written out as sums of non-negative terms; the k products of the inner sum and the five further operations add (k + 5) eps of the
     perturbed magnitudes.  u = R^-T rr then as in 2, with E' and |R^-T|.
  5. The apply pass z_e = gamma g_e + sum_j (u_j S_je + (gamma v_j) Y_je): the data terms dgamma |g_e| + du.|S_e| + (dgamma (|w| + dw) + gamma dw).|Y_e|,
     and every term passes through at most 2 k + 1 roundings (its product, 2 k additions), one more for gamma v_j and one to spare:
     (2 k + 3) eps (gamma^U |g_e| + u^U.|S_e| + gamma^U w^U.|Y_e|), the ^U magnitudes being |.| + d(.).
  6. The reference's own error: the two-loop coefficients (a, b) and the longdouble compact form's (-gamma w, u) differ by what extended
     precision leaves (2^-11 of the above at most); |b - u|.|S_e| + |a + gamma w|.|Y_e| is added to dz.
So dz_e = c_g |g_e| + c_S.|S_e| + c_Y.|Y_e| with non-negative coefficients that depend on the iteration only.  The safeguard's
g.z = gamma g.g + u.p - gamma w.q gets its bound dgz the same way ((k + 6) eps for its own operations).

THE BOUND ON x_{k+1}.  The projection is monotone, so the three device operations are followed on the interval [z - dz, z + dz]: u, d = P(u) - x,
t d and x + t d each widen their interval by eps of the result's magnitude (a fused t d + x rounds once less).  A component of the run's x_{k+1} is
accepted when it lies in the resulting interval.  Without a box the same four operations are followed as centre x - t z and radius: t dz plus
these few eps of |x|, |z| and |t z| (`free_step`; |z| through its upper bound gamma |g| + |a|.|Y| + |b|.|S|).  The reported ratio is
|x_{k+1} - midpoint| / half-width, a derived worst case: the assertion is ratio <= 1.

DISCRIMINATION.  An iteration whose largest half-width exceeds 1e-6 max_i |s_k,i| proves nothing; it is counted as skipped and not asserted.

The scalar checks ride along: gamma() within dgamma, stored_pairs() equal to the replayed count, updated[k] equal to s.y > DBL_EPSILON y.y in
longdouble wherever the difference clears its rounding bound, and an iteration whose resets() rose has g.z <= dgz and is predicted with z = g.
Each is reported as a ratio as well (a violated equality: inf), so `worst` covers everything.
"""
import hashlib

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
INF = float("inf")
CAP = 1e-6     # discrimination: half-width of x_{k+1} against max |s_k|
CHUNK = 1 << 15


class Recorder:
    """fn(x) -> (f, g) with every evaluation kept by the bytes of x: the replay uses the gradient the solver was handed and never re-evaluates.
    `order` is the sequence of evaluations, as keys; with keep_x the points themselves are kept beside it (tests/vec_replay.py reads both)."""

    def __init__(self, fn, keep_x=False):
        self.fn, self.seen, self.calls = fn, {}, 0
        self.order, self.points = [], ({} if keep_x else None)

    @staticmethod
    def _key(x):
        return hashlib.blake2b(np.ascontiguousarray(x, dtype=np.float64).tobytes(), digest_size=16).digest()

    def __call__(self, x):
        x = np.array(x, dtype=np.float64)
        f, g = self.fn(x)
        g = np.array(g, dtype=np.float64)
        self.calls += 1
        k = self._key(x)
        self.seen[k] = (float(f), g)
        self.order.append(k)
        if self.points is not None:
            self.points[k] = x
        return float(f), g.copy()

    def grad(self, x, what=""):
        k = self._key(x)
        if k not in self.seen:
            raise AssertionError(f"the objective was never evaluated at {what}: the replay has no gradient for it")
        return self.seen[k][1]


class Run:
    """what the replay needs of a run: settings, x_0 (projected), and per iteration x_{k+1}, t_k, updated[k] and the state seen after it"""

    def __init__(self, m, unit, lb, ub, x0, rec):
        self.m, self.unit, self.rec = m, unit, rec
        self.lb, self.ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
        self.x0 = np.minimum(np.maximum(np.asarray(x0, dtype=np.float64), self.lb), self.ub)
        self.xs, self.t, self.updated, self.states = [], [], [], []  # states: (stored_pairs, gamma, resets)

    def extend(self, xs, t, updated, states):
        assert len(xs) == len(t) == len(updated) == len(states), (len(xs), len(t), len(updated), len(states))
        self.xs += [np.array(x, dtype=np.float64) for x in xs]
        self.t += [float(v) for v in t]
        self.updated += [int(v) for v in updated]
        self.states += [(int(a), float(b), int(c)) for a, b, c in states]


def _chunks(n):
    return [slice(i, min(n, i + CHUNK)) for i in range(0, n, CHUNK)]


def cross(left, right):
    """(L_i.R_j: longdouble sums of longdouble products, |L_i|.|R_j|: float64) of float64 vectors, in one sweep with no temporary beyond a chunk"""
    ex, mag = np.zeros((len(left), len(right)), dtype=LD), np.zeros((len(left), len(right)))
    for c in _chunks(right[0].size):
        rl, ra = [r[c].astype(LD) for r in right], [np.abs(r[c]) for r in right]
        for i, l in enumerate(left):
            ll, la = l[c].astype(LD), np.abs(l[c])
            for j in range(len(right)):
                ex[i, j] += np.dot(ll, rl[j])
                mag[i, j] += np.dot(la, ra[j])
    return ex, mag.astype(LD)


class Memory:
    """the pairs (oldest first) as the float64 vectors the solver holds, with S'Y, Y'Y and their sums of magnitudes kept alongside"""

    def __init__(self, m):
        self.m, self.S, self.Y = m, [], []
        self.sy = self.yy = self.asy = self.ayy = np.zeros((0, 0), dtype=LD)

    def __len__(self):
        return len(self.S)

    def clear(self):
        self.__init__(self.m)

    def commit(self, s, y, sy, yy, asy):
        """-> True when the oldest pair was dropped"""
        dropped = len(self.S) == self.m
        if dropped:
            self.S, self.Y = self.S[1:], self.Y[1:]
            self.sy, self.yy, self.asy, self.ayy = (a[1:, 1:] for a in (self.sy, self.yy, self.asy, self.ayy))
        k = len(self.S)
        grown = []
        for a in (self.sy, self.yy, self.asy, self.ayy):
            b = np.zeros((k + 1, k + 1), dtype=LD)
            b[:k, :k] = a
            grown.append(b)
        self.sy, self.yy, self.asy, self.ayy = grown
        if k:
            col, acol = cross(self.S + self.Y, [y])     # S_j.y_p, Y_j.y_p
            row, arow = cross([s], self.Y)              # s_p.Y_j
            self.sy[:k, k], self.asy[:k, k] = col[:k, 0], acol[:k, 0]
            self.sy[k, :k], self.asy[k, :k] = row[0], arow[0]
            self.yy[:k, k] = self.yy[k, :k] = col[k:, 0]
            self.ayy[:k, k] = self.ayy[k, :k] = acol[k:, 0]
        self.sy[k, k], self.yy[k, k], self.asy[k, k], self.ayy[k, k] = sy, yy, asy, yy
        self.S, self.Y = self.S + [s], self.Y + [y]
        return dropped


def _closed(mat, a):
    """the smallest d >= 0 with d >= a + mat d (mat, a >= 0), or None when there is none to be had: d = (I - mat)^-1 a, verified"""
    mat, a = np.asarray(mat, dtype=np.float64), np.asarray(a, dtype=np.float64)
    if not (np.all(np.isfinite(mat)) and np.all(np.isfinite(a))):
        return None
    try:
        d = np.linalg.solve(np.eye(a.size) - mat, a)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(d)) or np.any(d < 0.0):
        return None
    d = d * (1.0 + 1e-9) + 1e-300  # (the float64 solve's own error; verified next)
    if not np.all(d >= a + mat @ d * (1.0 - 1e-12)):
        return None
    return d.astype(LD)


def _upper_inverse(r):
    k = r.shape[0]
    inv = np.zeros((k, k), dtype=LD)
    for j in range(k):
        for i in range(j, -1, -1):
            acc = (LD(1) if i == j else LD(0)) - np.dot(r[i, i + 1:j + 1], inv[i + 1:j + 1, j])
            inv[i, j] = acc / r[i, i]
    return inv


def two_loop_coefficients(sy, yy, p, q, gamma):
    """the two-loop recursion on coefficients: z = gamma g + a.Y + b.S.  q-vector = g + a.Y during the first loop, r = gamma g + a.Y + b.S in the second."""
    k = len(p)
    a, b, alpha = np.zeros(k, dtype=LD), np.zeros(k, dtype=LD), np.zeros(k, dtype=LD)
    for i in range(k - 1, -1, -1):          # newest first: alpha_i = s_i.q / s_i.y_i, q -= alpha_i y_i
        alpha[i] = (p[i] + np.dot(sy[i, :], a)) / sy[i, i]
        a[i] -= alpha[i]
    a = gamma * a                           # r = gamma q
    for i in range(k):                      # oldest first: beta_i = y_i.r / s_i.y_i, r += (alpha_i - beta_i) s_i
        beta = (gamma * q[i] + np.dot(yy[i, :], a) + np.dot(sy[:, i], b)) / sy[i, i]
        b[i] += alpha[i] - beta
    return a, b


class Direction:
    """z = gamma g + a.Y + b.S (longdouble coefficients) and dz = c_g |g| + c_s.|S| + c_y.|Y| (inf: no bound), gamma +- dgamma, g.z +- dgz"""

    def __init__(self, mem, g, unit):
        k, n = len(mem), g.size
        self.k = k
        self.gamma, self.dgam, self.dgz, self.c_g, self.bounded = 1.0, 0.0, 0.0, 0.0, True
        self.a = self.b = self.c_s = self.c_y = np.zeros(0, dtype=LD)
        if k == 0:
            self.gz = cross([g], [g])[0][0, 0]
            return
        gn, gk = LD((n + 2) * EPS), LD((k + 2) * EPS)
        with np.errstate(all="ignore"):
            ex, mag = cross(mem.S + mem.Y + [g], [g])
            p, q, gg = ex[:k, 0], ex[k:2 * k, 0], ex[2 * k, 0]
            dp, dq = gn * mag[:k, 0], gn * mag[k:2 * k, 0]
            sy, yy = mem.sy, mem.yy
            if unit:
                gamma, dgam = LD(1), LD(0)
            else:
                gamma = sy[-1, -1] / yy[-1, -1]
                r = gn * (mem.asy[-1, -1] / abs(sy[-1, -1]) + 1) + LD(EPS)
                dgam = abs(gamma) * r / (1 - r) if r < 1 else LD(INF)
            self.a, self.b = two_loop_coefficients(sy, yy, p, q, gamma)
            rm, er, ew = np.triu(sy), gn * np.triu(mem.asy), gn * mem.ayy
            dg, edg = np.diag(sy).copy(), gn * np.diag(mem.asy)
            rinv = _upper_inverse(rm)
            arinv = np.abs(rinv)
            e1 = er + gk * (np.abs(rm) + er)
            w = rinv @ p
            rr = dg * w + gamma * (yy @ w) - gamma * q
            u = rinv.T @ rr
            self.gamma, self.dgam = float(gamma), float(dgam)
            self.gz = gamma * gg + np.dot(self.b, p) + np.dot(self.a, q)
            self.bounded, self.dgz = False, INF
            if not (np.all(np.isfinite(rinv)) and np.isfinite(dgam)):
                return
            dw = _closed(arinv @ e1, arinv @ (dp + e1 @ np.abs(w)))
            if dw is None:
                return
            wu, gu, qu, pu, wwu = np.abs(w) + dw, gamma + dgam, np.abs(q) + dq, np.abs(p) + dp, np.abs(yy) + ew
            drr = (edg * wu + np.abs(dg) * dw) + (dgam * (wwu @ wu) + gamma * (ew @ wu + np.abs(yy) @ dw)) + (dgam * qu + gamma * dq)
            drr = drr + LD((k + 5) * EPS) * ((np.abs(dg) + edg) * wu + gu * (wwu @ wu) + gu * qu)
            du = _closed(arinv.T @ e1.T, arinv.T @ (drr + e1.T @ np.abs(u)))
            if du is None:
                return
            uu = np.abs(u) + du
            rnd = LD((2 * k + 3) * EPS)
            self.c_g = float(dgam + rnd * gu)
            self.c_s = du + rnd * uu + np.abs(self.b - u)
            self.c_y = (dgam * wu + gamma * dw) + rnd * gu * wu + np.abs(self.a + gamma * w)
            ggu = gg * (1 + gn)
            dgz = (dgam * ggu + gamma * gn * gg) + (np.dot(du, pu) + np.dot(np.abs(u), dp)) + (dgam * np.dot(wu, qu) + gamma * (np.dot(dw, qu) + np.dot(np.abs(w), dq)))
            dgz = dgz + LD((k + 6) * EPS) * (gu * ggu + np.dot(uu, pu) + gu * np.dot(wu, qu)) + abs(self.gz - (gamma * gg + np.dot(u, p) - gamma * np.dot(w, q)))
            self.dgz = float(dgz)
            self.bounded = bool(np.all(np.isfinite(self.c_s)) and np.all(np.isfinite(self.c_y)) and np.isfinite(self.c_g))

    def plain(self):
        """z = g: no pair, or the safeguard cleared the memory"""
        self.k, self.gamma, self.dgam, self.c_g, self.bounded = 0, 1.0, 0.0, 0.0, True


def step_interval(x, z, dz, t, lb, ub):
    """[lo, hi] (longdouble) of x + t (P(x - z') - x) over |z' - z| <= dz, each of the four operations widened by eps of its result"""
    e = LD(EPS)

    def wide(lo, hi):
        return lo - e * np.abs(lo), hi + e * np.abs(hi)
    with np.errstate(invalid="ignore"):
        ulo, uhi = wide(x - (z + dz), x - (z - dz))
        dlo, dhi = wide(np.minimum(np.maximum(ulo, lb), ub) - x, np.minimum(np.maximum(uhi, lb), ub) - x)
        plo, phi = wide(t * dlo, t * dhi)
        return wide(x + plo, x + phi)


def free_step(x, xl, z, za, dz, t):
    """(centre, radius) of x + t ((x - z') - x) over |z' - z| <= dz without a box: the centre x - t z in longdouble, the radius in float64 from
    upper bounds of the magnitudes (za >= |z|), operation by operation as in step_interval -- t dz plus a few eps of |x|, |z| and |t z|"""
    e, t64, xa = EPS, float(t), np.abs(x)
    ur = dz + e * (xa + za + dz)            # u = fl(x - z')
    dr = ur + e * (za + ur)                 # d = fl(u - x)
    pr = t64 * dr + e * t64 * (za + dr)     # fl(t d)
    xr = pr + e * (xa + t64 * (za + dr) + pr)
    return xl - t * z, xr * (1.0 + 1e-12)   # (the radius is a sum of non-negative float64 terms: 1e-12 covers its own rounding)


def compare_step(d, mem, x, g, xn, t, lb, ub):
    """(worst ratio |x_next - midpoint| / half-width, largest half-width) over the elements, chunk by chunk"""
    ratio = bound = 0.0
    t, k = LD(t), d.k
    coef = np.concatenate(([LD(d.gamma)], d.a, d.b)).astype(LD)
    cmag, cerr = np.abs(coef).astype(np.float64), np.concatenate(([d.c_g], d.c_y, d.c_s)).astype(np.float64)
    for c in _chunks(x.size):
        xl = x[c].astype(LD)
        if k == 0:
            z, za, dz = g[c].astype(LD), np.abs(g[c]), np.zeros(xl.size)
        else:
            rows = [g[c]] + [y[c] for y in mem.Y] + [s[c] for s in mem.S]
            wide = np.empty((2 * k + 1, xl.size), dtype=LD)
            for i, r in enumerate(rows):
                wide[i, :] = r
            mags = np.abs(np.stack(rows))
            z, za, dz = np.dot(coef, wide), cmag @ mags * (1.0 + 1e-12), cerr @ mags
        if np.all(np.isinf(lb[c])) and np.all(np.isinf(ub[c])):
            mid, hw = free_step(x[c], xl, z, za, dz, t)
        else:
            lo, hi = step_interval(xl, z, dz, t, lb[c], ub[c])
            hw, mid = ((hi - lo) / 2).astype(np.float64) * (1.0 + 1e-12), (hi + lo) / 2
        err = np.abs(xn[c] - mid).astype(np.float64)
        with np.errstate(all="ignore"):
            ratio = max(ratio, float(np.max(np.where(hw > 0, err / np.where(hw > 0, hw, 1), np.where(err == 0, 0.0, INF)))))
        bound = max(bound, float(np.max(hw)))
    return ratio, bound


class Report:
    def __init__(self):
        self.ratios, self.asserted, self.problems = [], [], []
        self.skipped = self.commits = self.max_k = self.head_advances = self.resets = 0
        self.worst_cap = 0.0  # largest half-width / max |s| over the run

    @property
    def iterations(self):
        return len(self.ratios)

    @property
    def n_asserted(self):
        return sum(self.asserted)

    @property
    def worst(self):
        return max([r for r, a in zip(self.ratios, self.asserted) if a] + [r for _, r, _ in self.problems] + [0.0])

    def line(self, name):
        return (f"replay {name}: worst ratio {self.worst:.3e}, asserted {self.n_asserted}, skipped {self.skipped} of {self.iterations}, largest k {self.max_k}, "
                f"head advances {self.head_advances}, commits {self.commits}, resets {self.resets}, skipped at {[k for k, a in enumerate(self.asserted) if not a]}")


def replay(run):
    assert run.t and all(t > 0.0 for t in run.t), "the replay needs at least one iteration and positive steps"
    rep, mem = Report(), Memory(run.m)
    x, g = run.x0, run.rec.grad(run.x0, "x_0")
    resets = 0
    for k, (xn, t, upd, (stored, gam_dev, res_dev)) in enumerate(zip(run.xs, run.t, run.updated, run.states)):
        gnext = run.rec.grad(xn, f"x_{k + 1}")
        assert res_dev in (resets, resets + 1), (k, res_dev, resets)
        was_reset = res_dev > resets
        resets = res_dev
        d = Direction(mem, g, run.unit)
        rep.max_k = max(rep.max_k, len(mem))
        gz, dgz = float(d.gz), d.dgz
        if was_reset:  # taken as given; checked: g.z is not above its rounding bound (not finite counts as such)
            if not len(mem):
                rep.problems.append((k, INF, "a reset with an empty memory"))
            elif np.isfinite(gz) and np.isfinite(dgz) and gz > dgz:
                rep.problems.append((k, gz / dgz if dgz > 0.0 else INF, f"reset although g.z = {gz:.3e} > its bound {dgz:.3e}"))
            mem.clear()
            d.plain()
            rep.resets += 1
        elif len(mem) and np.isfinite(dgz) and gz < -dgz:
            rep.problems.append((k, -gz / dgz if dgz > 0.0 else INF, f"no reset although g.z = {gz:.3e} < -{dgz:.3e}"))
        if np.isfinite(d.dgam) and abs(gam_dev - d.gamma) > d.dgam:
            rep.problems.append((k, abs(gam_dev - d.gamma) / d.dgam if d.dgam > 0.0 else INF, f"gamma {gam_dev!r} against {d.gamma!r} +- {d.dgam:.3e}"))
        s = xn - x
        smax = float(np.max(np.abs(s)))
        ratio, bound = compare_step(d, mem, x, g, xn, t, run.lb, run.ub) if d.bounded else (INF, INF)
        asserted = not bound > CAP * smax
        rep.worst_cap = max(rep.worst_cap, bound / smax if smax > 0.0 else (0.0 if bound == 0.0 else INF))
        rep.ratios.append(ratio)
        rep.asserted.append(asserted)
        rep.skipped += 0 if asserted else 1
        # the pair, as the solver holds it, and the commit rule
        y = gnext - g
        ex, mag = cross([s, y], [y])
        sy, yy, asy = ex[0, 0], ex[1, 0], mag[0, 0]
        gn = LD((s.size + 2) * EPS)
        margin = sy - LD(EPS) * yy
        if abs(margin) > gn * asy + LD(EPS) * yy * (gn + 2 * LD(EPS)) and bool(upd) != bool(margin > 0):
            rep.problems.append((k, INF, f"updated = {upd} although s.y - eps y.y = {float(margin):.3e}"))
        if upd:
            rep.commits += 1
            rep.head_advances += 1 if mem.commit(s, y, sy, yy, asy) else 0
        if stored != len(mem):
            rep.problems.append((k, INF, f"stored_pairs() = {stored}, replayed {len(mem)}"))
        x, g = xn, gnext
    return rep


def check(rep, name):
    """the assertion of both tests: every asserted iteration and every scalar check inside its bound"""
    print(rep.line(name))
    assert not rep.problems, (name, rep.problems[:3])
    bad = [(k, r) for k, (r, a) in enumerate(zip(rep.ratios, rep.asserted)) if a and not r <= 1.0]
    assert not bad, (name, bad[:5])
