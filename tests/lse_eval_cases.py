"""The log-sum-exp evaluation INSIDE a solver run, held to extended precision: what tests/test_ref_lse_eval.py (CPU, licenses the checker on float64
restatements and on planted faults) and tests/test_gpu_lse_eval.py (GPU) share.  Test infrastructure: the product does not import this file.

    f(x) = log sum_k exp(a_k'x + c_k) + mu/2 x'x,        g(x) = A'p + mu x,   p = softmax(Ax + c)

is evaluated on the device by a running-maximum softmax in three implementations (lse_onepass/combine/finish1, qn_kernels.hip.h; s2g_onepass/
s2g_combine/s2g_vec with the rank weighting of the GOBJ prologue, qn_sym2g.hip.h and qn_sym2.hip.h; the two-pass form behind QN_LSE_TWO_PASS=1).
Here are the problems that reach what benign data does not (rescale factors that underflow, maxima that rise at every row, ranks and workgroups
without rows, masked rows c_k = -inf), the np.longdouble truth with derived bounds, and the replay of a run from its own recorded iterates.

THE GRID (qn_logsumexp_create, lse_onepass_kernel).  A rank owns mrpr = 16 ceil(ceil(m / P) / 16) consecutive rows (the last ranks fewer, or none:
m = 20 on 4 ranks leaves ranks 2 and 3 empty), dealt to G = max(1, min(256, ceil(mrpr / 4))) workgroups of ceil(mrpr / G) rows; since mrpr is a
multiple of 16 that is 4 rows per workgroup up to mrpr = 1024 (m = 5: one workgroup of 4 rows, one of 1, two without rows; m = 1030: 206
workgroups of 5 rows, 50 without).  A workgroup folds a running (m, S, G) row by row, the workgroups are combined with exp(m_w - m_r), the ranks
with exp(m_r - M) in rank order.  `grid` and `eval_fold` restate exactly that; eval_fold is the specification for -inf rows.

MASKED ROWS.  A row with c_k = -inf contributes nothing, wherever it falls in that partition: the truth of a masked problem is the truth of the
problem with those rows deleted.  (+inf and NaN in c and non-finite entries of A are out of scope.)

THE BOUNDS at a point x, for a float64 evaluation in ANY summation order, with or without fused multiply-adds, through any number of running
rescales.  eps = 2^-52, twice the unit roundoff (the factor of two pays for second-order terms and for evaluating the bound in floating point).
  1. z_k = a_k'x + c_k: a sum of n products in any order carries (n + 2) eps of the sum of magnitudes, the addition of c_k one more:
         |dz_k| <= dz = 1.001 (n + 3) eps Z,     Z = max_k (sum_j |a_kj x_j| + |c_k|) over the unmasked rows
     (1.001: the longdouble truth's own n 2^-63 Z).
  2. A row enters S as the product of exp(z_k - m) at the running maximum m of its moment and of every later rescale exp(m - m'), exp(m_w - m_r),
     exp(m_r - M).  The exponents telescope to z_k - M; each argument is rounded once (eps |difference|; along a chain of rising maxima the
     differences add up to at most 2 Z, the three chains together 6 eps Z), each exp is good to 2 eps, each product and each addition of the
     non-negative partial sums to eps: at most 4 per row of the workgroup, G + 2 for the workgroups, P + 2 for the ranks.  With 4 rows' worth per
     row of A, G <= 256 and P <= 32:
         every term of S, and of G_j = sum_k w_k a_kj, carries a relative error th <= (6 Z + 4 m + 300) eps    on top of exp(dz_k).
     A factor that underflows loses a term whose true weight is below 1e-290 of S: an absolute 1e-280 covers it.
  3. f.  M^ + log S^ = log sum_k exp(z^_k)(1 + th_k) = lse(z^) + log(1 + th'), |th'| <= th, and log-sum-exp is 1-Lipschitz in max_k |dz_k|.
     S lies in [1 - th, m], so log S <= log m; the logarithm (2 eps), M + log S, mu/2 x'x (n + 4 roundings of positive terms) and the last
     addition (or the table's 1/2 tot0 - tot1) add 4 eps (Z + log m + 1) + (n + 6) eps mu/2 x'x:
         |f^ - f| <= bf = dz + 1.01 th + 4 eps (Z + log m + 1) + (n + 6) eps mu/2 x'x + 1e-280.
  4. g.  p^_k / p_k = exp(dz_k)(1 + th_k) / (sum_i p_i exp(dz_i)(1 + th_i)): a relative error of at most 2.02 (dz + th) while dz + th < 0.01
     (asserted) -- the softmax weights' 2 max |dz| + O(m) eps.  The division by S, mu x_j and the last addition add 4 eps of the scale:
         |g^_j - g_j| <= bg_j = (2.02 (dz + th) + 4 eps) ((|A|'p)_j + mu |x_j|) + 1e-280.
Nothing in these constants is tuned against a device; tests/test_ref_lse_eval.py prints how far inside three float64 orders sit.

WHICH POINT A TRACE FIELD BELONGS TO (qn_ctl_step.hip.h: qn_st_check sets tr_f = f_k and tr_gnorm = sqrt(gg) at the loop top, before the line
search; qn_st_after_next sets s_norm, y_norm from the accepted point's staged sums and toggles x <- x+; qn_st_iter_end writes the record, and the
prologue copies the iterate only then).  Record k holds f = f(x_k), gnorm = ||g(x_k)||, t = t_k, s_norm = ||x_{k+1} - x_k||,
y_norm = ||g(x_{k+1}) - g(x_k)||, updated = whether the pair (s_k, y_k) went into H, and the recorded iterate xs[k] is x_{k+1}; x_0 is the caller's.

THE REPLAY (tests/qn_replay.py, shared with the quadratic objective's tests/quad_replay_cases.py; `replay` below hands it this objective's truth)
checks every recorded iteration on its own, from the run's own iterates, so nothing accumulates:
  f       |trace.f - f(x_k)| <= bf(x_k);
  gnorm   against ||g(x_k)||: ||bg(x_k)||_2 for the gradient, (n + 2) eps relative for the sum of squares and eps for the square root;
  s_norm  against ||fl(x_{k+1} - x_k)||_2 (the library forms s with one subtraction: exact apart from the sum);
  y_norm  against ||g(x_{k+1}) - g(x_k)||_2, both gradients' bounds and the subtraction's eps as absolute error; where that exceeds 1e-3 of
          y_norm the iteration proves nothing about y and is counted as skipped;
  dir     entry by entry, x_{k+1} - x_k against -t_k H_k g_k.  H_k is rebuilt in longdouble from H_0 = I and the replayed pairs
          s_i = fl(x_{i+1} - x_i), y_i = g(x_{i+1}) - g(x_i) (truth), i < k, updated[i] taken as given, with the rank-2 form of DESIGN.md 2:
              u = H y,   H+ = H + c_ss s s' + c_su (s u' + u s') + c_uu u u',
              DFP: c_ss = 1 / s'y, c_uu = -1 / y'u;     BFGS: c_ss = (1 + y'u / s'y) / s'y, c_su = -1 / s'y.
          The half-width of entry j:
              t_k (|H_k| bg(x_k))_j  +  (n + 4) eps t_k (|H_k| |g_k|)_j  +  t_k (DH_k (|g_k| + bg(x_k)))_j  +  2 eps (|x_k|_j + |x_{k+1}|_j).
          DH_k bounds |H_k of the device - H_k| entry by entry: the device's y_i differ from the truth's by dy_i = bg(x_{i+1}) + bg(x_i) + eps |y_i|,
          hence u by du = DH |y| + |H| dy + (n + 4) eps Habs |y|, the inner products s'y and y'u by sums of such magnitudes, the coefficients by
          d(1 / a) = da / (|a| (|a| - da)), and every term of the formula by (|a| + da)(|b| + db) - |a| |b| written out as sums of non-negative
          terms; the device's own rounding of coefficients and of the stored H adds 8 eps Habs, Habs = I + sum |c| |.||.|' being the formula with every
          term taken in magnitude (it also covers the lazy form d = -(v + al s + be u) in which the device applies a pending update).
          Only the first REPLAY = 3 iterations (H_k costs n^2 longdoubles); above n = 4224 only iteration 0 (H_0 = I, d = -g).
          Discrimination, as lbfgs_replay.CAP: an iteration whose largest half-width exceeds 1e-6 max_j |s_k,j| is skipped, not asserted.
Every check is a ratio |error| / bound; the assertion is ratio <= 1.  At most 10 % of the (case, iteration, check) triples may be skipped, no case
may have every direction check skipped, iteration 0 of every case is asserted (`Tally`)."""
import functools
import math

import numpy as np

import qn_replay
from qn_replay import (CAP, CHECKS, EPS, INF, LD, REPLAY, SKIP_SHARE, Y_CAP, InverseHessian, Report, Tally, _ratio, check, coefficients,  # noqa: F401
                       point_ratios)

MU = 0.1
REPLAY_N = 4224      # above: iteration 0 only


# ---- the grid ----
def rows_per_rank(m, world):
    per = -(-m // world)
    return max(16, -(-per // 16) * 16)


def grid(m, world):
    """(mrpr, G, rows per workgroup) of a rank of `world`"""
    mrpr = rows_per_rank(m, world)
    g = max(1, min(256, (mrpr + 3) // 4))
    return mrpr, g, -(-mrpr // g)


def workgroup_rows(m, world, rank, w):
    """the global rows [lo, hi) of workgroup w of `rank` (empty: lo >= hi)"""
    mrpr, g, per = grid(m, world)
    lo = rank * mrpr + w * per
    return lo, min(rank * mrpr + min(mrpr, (w + 1) * per), m)


# ---- the problems ----
class Case:
    def __init__(self, name, m, n, family, param=None, worlds=(1,), rpr=None, mask_world=1, seed=17):
        self.name, self.m, self.n, self.family, self.param, self.worlds, self.rpr, self.mask_world, self.seed = name, m, n, family, param, worlds, rpr, mask_world, seed
        self.iters = 1 if n > REPLAY_N else 3

    def __repr__(self):
        return self.name

    @property
    def label(self):
        return self.family + ("" if self.param is None else f"({self.param:g})")


def mask_of(m, world):
    """the stated index set of a masked case laid out for `world` ranks: the first row of workgroup 0, every row of one middle workgroup (of rank 0),
    the last row, and on more than one rank every row of rank 1"""
    mrpr, g, per = grid(m, world)
    own = min(mrpr, m)                      # rows of rank 0
    nwg = -(-own // per)                    # its workgroups that have rows
    rows = {0, m - 1}
    if nwg >= 3:
        lo, hi = workgroup_rows(m, world, 0, nwg // 2)
        rows |= set(range(lo, hi))
    if world > 1:
        rows |= set(range(mrpr, min(2 * mrpr, m)))
    assert len(rows) < m
    return sorted(rows)


# (m, n): the smallest shapes at which each mechanism exists -- one row; two workgroups; empty ranks (m = 20: mrpr = 16 on 2, 3 and 4 ranks);
# KCH = 2 with the clamped tail column pair (n = 1152); 256 workgroups, 50 of them without rows (m = 1030); KCH = 4, 8, 16 (n = 2176, 4224, 16384).
# Row-sharded runs take the second-generation structure when every rank owns whole 128-blocks of H, n / P a multiple of 128: two and four ranks get
# n = 1024 and, for KCH = 2, n = 1536 (the tail column pair is clamped there as well); three ranks n = 1152.
CASES = [
    Case("m1_n1024_normal1", 1, 1024, "normal", 1.0),
    Case("m5_n1024_normal300", 5, 1024, "normal", 300.0),
    Case("m5_n1024_masked", 5, 1024, "masked"),
    Case("m5_n1024_desc5", 5, 1024, "desc", 5.0),
    Case("m20_n1024_normal1", 20, 1024, "normal", 1.0, worlds=(1, 2, 4)),
    Case("m20_n1152_normal3000", 20, 1152, "normal", 3000.0, worlds=(3,)),
    Case("m20_n1024_offset20", 20, 1024, "rank_offset", 20.0, worlds=(1, 2, 4), rpr=16),
    Case("m20_n1152_offset20", 20, 1152, "rank_offset", 20.0, worlds=(3,), rpr=16),
    Case("m20_n1024_offset800", 20, 1024, "rank_offset", 800.0, worlds=(1, 2, 4), rpr=16),
    Case("m20_n1152_offset800", 20, 1152, "rank_offset", 800.0, worlds=(3,), rpr=16),
    Case("m20_n1024_masked", 20, 1024, "masked", worlds=(1,)),
    Case("m20_n1024_masked_ranks", 20, 1024, "masked", worlds=(1, 2, 4), mask_world=2),
    Case("m20_n1152_masked_ranks", 20, 1152, "masked", worlds=(3,), mask_world=3),
    Case("m300_n1152_asc5", 300, 1152, "asc", 5.0),
    Case("m300_n1536_asc5", 300, 1536, "asc", 5.0, worlds=(2,)),
    Case("m300_n1152_desc5", 300, 1152, "desc", 5.0, worlds=(1, 3)),
    Case("m300_n1152_normal3000", 300, 1152, "normal", 3000.0),
    Case("m300_n1536_normal3000", 300, 1536, "normal", 3000.0, worlds=(4,)),
    Case("m300_n1536_offset20_r80", 300, 1536, "rank_offset", 20.0, worlds=(1, 4), rpr=80),
    Case("m300_n1152_offset800_r112", 300, 1152, "rank_offset", 800.0, worlds=(3,), rpr=112),
    Case("m300_n1536_offset20_r160", 300, 1536, "rank_offset", 20.0, worlds=(2,), rpr=160),
    Case("m300_n1152_masked_ranks", 300, 1152, "masked", worlds=(1, 3), mask_world=3),
    Case("m1030_n1152_normal300", 1030, 1152, "normal", 300.0),
    Case("m1030_n1152_masked", 1030, 1152, "masked"),
    Case("m5_n2176_asc5", 5, 2176, "asc", 5.0),
    Case("m5_n4224_normal300", 5, 4224, "normal", 300.0),
    Case("m5_n4224_masked", 5, 4224, "masked"),
    Case("m5_n16384_normal1", 5, 16384, "normal", 1.0),
]
BY_NAME = {c.name: c for c in CASES}
SHARDED = [(c, w) for c in CASES for w in c.worlds if w > 1]


@functools.lru_cache(maxsize=None)
def problem(name):
    """(a, c, x0) of the case, read-only: a = 3 / sqrt(n) N(0, 1), x0 = N(0, 1); the spread is in c (scaling x would let mu/2 ||x||^2 and mu x
    drown the softmax part)"""
    cs = BY_NAME[name]
    rng = np.random.default_rng(cs.seed)
    a = rng.standard_normal((cs.m, cs.n)) * (3.0 / np.sqrt(cs.n))
    x0 = rng.standard_normal(cs.n)
    base = rng.standard_normal(cs.m)
    k = np.arange(cs.m, dtype=np.float64)
    if cs.family == "normal":
        c = base * cs.param
    elif cs.family == "asc":
        c = cs.param * k
    elif cs.family == "desc":
        c = -cs.param * k
    elif cs.family == "rank_offset":
        c = base - cs.param * (np.arange(cs.m) // cs.rpr)
    elif cs.family == "masked":
        c = base.copy()
        c[mask_of(cs.m, cs.mask_world)] = -INF
    else:
        raise ValueError(cs.family)
    for v in (a, c, x0):
        v.setflags(write=False)
    return a, c, x0


# ---- truth and bounds ----
class Truth:
    """f, g (longdouble) at x with the bounds bf, bg (float64) of the module docstring; z, p of the unmasked rows ride along"""

    def __init__(self, a, c, x, mu=MU):
        m, n = a.shape
        keep = np.flatnonzero(c > -INF)
        assert keep.size and np.all(np.isfinite(c[keep])) and np.all(np.isfinite(x))
        xl, xa = x.astype(LD), np.abs(x)
        z, zk = np.empty(keep.size, dtype=LD), np.empty(keep.size)
        for i in range(0, keep.size, 128):  # chunk by chunk: no longdouble copy of A
            rows = keep[i:i + 128]
            z[i:i + 128] = a[rows].astype(LD) @ xl + c[rows].astype(LD)
            zk[i:i + 128] = np.abs(a[rows]) @ xa + np.abs(c[rows])
        self.keep, self.z = keep, z
        self.zcap = float(zk.max()) * (1.0 + 1e-12)
        big = z.max()
        e = np.exp(z - big)
        ssum = e.sum()
        self.p = e / ssum
        xx = np.dot(xl, xl)
        self.f = big + np.log(ssum) + LD(mu) * xx / 2
        g, scale = LD(mu) * xl, mu * xa
        p64 = self.p.astype(np.float64)
        for i in range(0, keep.size, 128):
            rows = keep[i:i + 128]
            g = g + a[rows].astype(LD).T @ self.p[i:i + 128]
            scale = scale + np.abs(a[rows]).T @ p64[i:i + 128]
        self.g, self.scale = g, scale * (1.0 + 1e-12)
        self.dz = 1.001 * (n + 3) * EPS * self.zcap
        self.th = (6.0 * self.zcap + 4.0 * m + 300.0) * EPS
        assert self.dz + self.th < 0.01, (self.dz, self.th)
        self.bf = self.dz + 1.01 * self.th + 4.0 * EPS * (self.zcap + math.log(m) + 1.0) + (n + 6) * EPS * 0.5 * mu * float(xx) + 1e-280
        self.bg = (2.02 * (self.dz + self.th) + 4.0 * EPS) * self.scale + 1e-280
        self.gnorm = float(np.sqrt(np.dot(g, g)))
        self.bgnorm = float(np.linalg.norm(self.bg))


# ---- float64 restatements of the evaluation, three orders ----
def eval_plain(a, c, x, mu=MU):
    z = a @ x + c
    big = z.max()
    e = np.exp(z - big)
    s = e.sum()
    return big + math.log(s) + 0.5 * mu * (x @ x), a.T @ (e / s) + mu * x


def eval_reversed(a, c, x, mu=MU):
    """every sum from the far end, one term at a time"""
    rev = slice(None, None, -1)
    z = np.add.accumulate((a * x)[:, rev], axis=1)[:, -1] + c
    big = z.max()
    e = np.exp(z - big)
    s = float(np.add.accumulate(e[rev])[-1])
    p = e / s
    g = np.add.accumulate((a * p[:, None])[rev], axis=0)[-1] + mu * x
    return big + math.log(s) + 0.5 * mu * float(np.add.accumulate((x * x)[rev])[-1]), g


def _exp(v):
    return math.exp(v) if v == v else float("nan")


def eval_fold(a, c, x, world=1, mu=MU, select=True, fault=None):
    """The kernels' fold (module docstring, THE GRID), float64.  select=False: the row loop before the -inf rule (exp(m_run - m_new) with both -inf).
    fault: a planted defect -- ("drop", k) row k left out; ("no_rescale_g",) G not rescaled when the maximum rises; ("rank_weight_one", r) rank r's
    weight left at 1; ("stale_empty_rank",) a rank without rows folded in from a slot never written, (m_r, S_r) = (0, 1); ("f_without_max",)."""
    m, n = a.shape
    fault = fault or ("none",)
    mrpr, nwg, per = grid(m, world)
    ranks = []
    for r in range(world):
        wgs = []
        for w in range(nwg):
            lo, hi = workgroup_rows(m, world, r, w)
            m_run, s_run, g_run = -INF, 0.0, np.zeros(n)
            for k in range(lo, hi):
                if fault == ("drop", k):
                    continue
                z = float(a[k] @ x) + float(c[k])
                m_new = max(m_run, z)
                m_ref = 0.0 if (select and m_new == -INF) else m_new
                scale, e = _exp(m_run - m_ref), _exp(z - m_ref)
                s_run = s_run * scale + e
                g_run = (g_run if fault[0] == "no_rescale_g" else g_run * scale) + e * a[k]
                m_run = m_new
            wgs.append((m_run, s_run, g_run))
        m_r = max(w[0] for w in wgs)
        s_r, g_r = 0.0, np.zeros(n)
        for m_w, s_w, g_w in wgs:  # (a workgroup without rows is skipped)
            if m_w != -INF:
                fac = _exp(m_w - m_r)
                s_r, g_r = s_r + s_w * fac, g_r + g_w * fac
        if m_r == -INF and fault[0] == "stale_empty_rank":
            m_r, s_r = 0.0, 1.0
        ranks.append((m_r, s_r, g_r))
    big = max(r[0] for r in ranks)
    s, g = 0.0, np.zeros(n)
    for r, (m_r, s_r, g_r) in enumerate(ranks):  # ranks in rank order; a rank without rows contributes nothing
        if m_r != -INF:
            wr = 1.0 if fault == ("rank_weight_one", r) else _exp(m_r - big)
            s, g = s + s_r * wr, g + g_r * wr
    f = (0.0 if fault[0] == "f_without_max" else big) + (math.log(s) if s > 0 else (-INF if s == 0 else float("nan"))) + 0.5 * mu * float(x @ x)
    with np.errstate(all="ignore"):
        return f, g / s + mu * x


# ---- a float64 DFP / BFGS run on a restatement (backtracking, the rank-2 form) ----
def reference_run(ev, x0, method, iters, perturb=None, tol=1e-10):
    """-> (trace records, xs) in the library's layout.  ev(x) -> (f, g).  perturb = (k, j, rel): entry j of the gradient the direction of iteration k
    is formed from is off by rel |g_j| (a wrong entry of the staged g+ that no sum sees)."""
    n = x0.size
    x = np.array(x0, dtype=np.float64)
    f, g = ev(x)
    h = None
    tr, xs = [], []
    for k in range(iters):
        if math.sqrt(g @ g) < tol or (tr and (tr[-1]["s_norm"] < tol or tr[-1]["y_norm"] < tol)):  # has_converged at the loop top (bfgs.rs:64-76)
            break
        gd = g.copy()
        if perturb and perturb[0] == k:
            gd[perturb[1]] += perturb[2] * abs(gd[perturb[1]])
        d = -gd if h is None else -(h @ gd)
        gd0, t, evals = float(g @ d), 1.0, 0
        for _ in range(60):
            ft, _g = ev(x + t * d)
            evals += 1
            if math.isfinite(ft) and ft - f <= 1e-4 * t * gd0:
                break
            t *= 0.5
        xn = x + t * d
        fn, gn = ev(xn)
        s, y = xn - x, gn - g
        rec = dict(f=f, gnorm=float(np.sqrt(g @ g)), t=t, s_norm=float(np.sqrt(s @ s)), y_norm=float(np.sqrt(y @ y)), updated=1, n_evals=evals + 1)
        if k + 1 < iters and n <= REPLAY_N:
            if h is None:
                h = np.eye(n)
            u = h @ y
            css, csu, cuu = coefficients(method, float(s @ y), float(y @ u))
            h += css * np.outer(s, s) + csu * (np.outer(s, u) + np.outer(u, s)) + cuu * np.outer(u, u)
        tr.append(rec)
        xs.append(xn)
        x, f, g = xn, fn, gn
    return tr, np.array(xs)


# ---- the replay (tests/qn_replay.py: Report, InverseHessian, Tally, check) with this objective's truth ----
def replay(name, a, c, x0, method, tr, xs, mu=MU, truth_cache=None):
    """Report of a run: tr the trace records (f, gnorm, t, s_norm, y_norm, updated), xs[k] = x_{k+1}"""
    cache = truth_cache if truth_cache is not None else {}

    def truth(x):
        key = x.tobytes()
        if key not in cache:
            cache[key] = Truth(a, c, x, mu)
        return cache[key]

    return qn_replay.replay(name, truth, x0, method, tr, xs, iters=REPLAY if a.shape[1] <= REPLAY_N else 1, kind="lse")
