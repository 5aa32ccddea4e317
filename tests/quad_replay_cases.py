"""Dense quasi-Newton runs on device quadratics, replayed in extended precision: what tests/test_ref_quad_replay.py (CPU: licenses the checker on
float64 restatements in three summation orders and on ten planted faults) and tests/test_gpu_quad_replay.py (GPU) share.  Test infrastructure: the
product does not import this file.  The replay itself is tests/qn_replay.py.

    f(x) = 1/2 x'Qx - b'x,        g(x) = Qx - b        (Q multiplied AS GIVEN: for the non-symmetric case g is not the gradient of f; the kernels
                                                        and this truth agree on that)

THE TRUTH at a point x is formed in np.longdouble.  THE BOUNDS hold for a float64 evaluation in ANY summation order, with or without fused
multiply-adds, padded or not (a padded product is an exact 0 and adding it is exact).  eps = 2^-52, twice the unit roundoff.
  g_j.  A product Q_ji x_i is rounded once (not at all inside an FMA), then passes through additions on its way into the row sum.  However the sum
        is bracketed -- the row kernels' chunk loop (one FMA chain of n_pad / 256 pairs per thread, qn_block_fold's LDS tree over the 256 threads;
        chunks_per_trip only changes how many loads are in flight, the chain per thread is the same), the symmetric tiles' per-block partial sums
        of direct and mirrored contributions and their fold over the block-row (qn_sym.hip.h, qn_sym2.hip.h, s2_evalr's mover / multiplier waves),
        the rank-order sum of a row-sharded run's partial vectors -- a sum of n terms has n - 1 additions, and no product passes through more than
        all of them.  The subtraction of b_j is one more: at most n + 1 roundings; two more pay for second-order terms and for evaluating the
        bound itself in floating point, n + 3 <= c_g(n) = n + 4:
            |g^_j - g_j| <= bg_j = 1.001 (n + 4) eps ((|Q| |x|)_j + |b_j|).
  f.    The kernels form f = 1/2 tot0 - tot1 (s2_hreduce and the control step's table; the row kernels' partial columns x+.q and b.x+), tot0 the sum
        of x_i q^_i with q^_i the row sum above.  A product Q_ij x_j goes through at most n roundings into q^_i, one for x_i q^_i, n - 1 additions of
        tot0 (per-workgroup partial sums, their fold, the ranks: one sum of n terms again), the halving is exact, the last subtraction one more:
        2 n + 1, plus two, 2 n + 3 <= c_f(n) = 2 n + 8; a product b_i x_i goes through n + 1.  With every term taken in magnitude:
            |f^ - f| <= bf = 1.001 c_f(n) eps (1/2 |x|'|Q||x| + |b|'|x|).
  1.001: the longdouble truth's own error, the same expressions with 2^-64.  c_g and c_f follow from the count above alone (each with the same
  margin of two roundings and rounded up); nothing is tuned against a device.  tests/test_ref_quad_replay.py prints how far inside three
  float64 orders sit (worst ratio of any check on any case: 1.3e-1, a direction of the wide problem; 8.3e-2 on the seeded problems, no check skipped).

THE PROBLEMS.  `synth`: the project's seeded SPD quadratic (tests/problems.py synth_problem, kappa = 100) where the oracle library is at hand, a
seeded numpy SPD matrix of the same shape (uniform off-diagonal entries / n, the same diagonal) otherwise.  `nonsym`: the same with a strictly upper
triangular perturbation of relative size 1e-3 -- the library must take the full-matrix row kernels.  `wide`: Q = D M D with M the seeded matrix and
D = diag(10^(+-3)) in a seeded order, entries spanning 1e-6 .. 1e6 in magnitude, so that |Q||x| dominates |Qx| in the rows of small scale.
THE BOX (`box`) at x0: entries j = 0 mod 4 lie below their lower bound, j = 1 mod 4 above their upper bound, j = 2 mod 4 are free inside finite
bounds and j = 3 mod 4 have no bounds at all.  A bounded solver starts from P(x0).

THE SIZES, each the smallest at which its mechanism exists (qn_host_minimize.hip.h, the shapes the symmetric paths need; QN_TB = 128, the fused
path's n > 5, symmetric storage from n_pad >= 1024):
    7     row kernels, n_pad = 16, one ragged tile            130   row kernels, n_pad = 144: padded rows and columns stay out of every sum
    1000  n_pad = 1008 < 1024: row kernels on many workgroups (also with chunks_per_trip 2 and 4)
    1020  n_pad = 1024 != n: first-generation symmetric tiles with four padded rows / columns
    1024  second generation, nb = 8                           1152  nb = 9, odd                    4096  nb = 32, the G = 256 instantiations

SEGMENT PLANS.  A run is a sequence of minimize calls on one solver; with `read_h` the inverse Hessian is read between the calls (the getter
flushes what is pending) and every call is replayed as one segment from the matrix just read; without, the calls are replayed as ONE run from
H_0 = I (the warm continuation).  With the store-skip on, (3, 3) ends its calls with one pending update behind a stored pass, (1, 2, 3) with none
stored yet / two pending / one, (2, 2, 2) with two pending every time.

DETECTION, measured against the float64 restatement only (test_ref_quad_replay.py::test_detection_thresholds_of_a_wrong_gradient_entry, BFGS,
one segment of three from I, the seeded problem in the tile order): the smallest relative error of the entry of largest |g| of the gradient a
direction is formed from that is still rejected --
    n = 7    (grid of half decades):  iteration 0: 1e-14,  iteration 1: 3.2e-13,  iteration 2: 1e-12
    n = 130  (grid of half decades):  iteration 0: 1e-13,  iteration 1: 1e-12,    iteration 2: 3.2e-12
    n = 1000 (grid of decades):       iteration 0: 1e-12,  iteration 1: 1e-11,    iteration 2: 1e-10
    n = 1024 (grid of decades):       iteration 0: 1e-12,  iteration 1: 1e-11,    iteration 2: 1e-10
(the seeded matrix being the oracle library's; the tally test prints which matrix a run used)
a factor of 3 to 10 lost per replayed iteration, which is why segments restart from a matrix read back.  The asserted size is the fixed 1e-9
(test_fault_1: n = 7, 130, 1024, iterations 0 .. 2 of both segments of plan (3, 3)): the norm-wise tolerance of the parity tests, entry by entry.

ON THE GPU (one MI355X; the last test of tests/test_gpu_quad_replay.py prints the record, which is no tolerance), worst asserted ratio per path:
    path                                   f        gnorm    s_norm   y_norm   dir      H
    row kernels n = 7                      2.3e-2   3.4e-2   8.9e-2   2.8e-2   5.7e-2   3.3e-2
    row kernels n = 130                    3.1e-3   3.2e-3   7.1e-3   2.5e-3   3.3e-2   5.9e-2
    row kernels n = 1000 (1, 2, 4 chunks)  3.8e-4   4.4e-4   9.3e-4   2.7e-4   9.5e-3   7.4e-2
    first-generation tiles n = 1020        3.4e-4   4.7e-4   9.5e-4   3.2e-4   9.4e-3   7.3e-2
    second generation n = 1024 (+ options: second_generation, symmetric_storage, hpass_store_skip, sync)
                                           5.1e-4   4.5e-4   9.2e-4   2.8e-4   1.1e-2   7.1e-2
    second generation n = 1152             2.4e-4   3.7e-4   8.6e-4   3.4e-4   8.5e-3   7.5e-2
    second generation n = 4096 (+ row_slivers, eval_pair_instance, eval_mover_multiplier, eval_zigzag off; one segment of three each)
                                           1.1e-4   7.2e-5   1.2e-4   6.1e-5   2.8e-3   7.1e-2
    box n = 1024, both bounded paths       5.0e-4   4.8e-4   9.4e-4   4.6e-4   4.5e-3   7.7e-2
    box n = 4096 (BFGSB / SR1B + BackTrackingB, projection in the kernel and per launch; SR1B / DFPB + MoreThuenteB; one segment of three)
                                           1.2e-4   1.1e-4   2.3e-4   4.6e-5   2.3e-3   6.6e-2
    2 / 3 / 4 ranks                        3.8e-4   4.5e-4   9.3e-4   4.3e-4   1.1e-2   7.5e-2
    host closure n = 1020, 1024            0        9.5e-4   9.5e-4   6.2e-4   1.0e-1   6.8e-2
    non-symmetric Q n = 1024               2.6e-4   4.5e-4   7.3e-4   3.8e-4   1.1e-2   6.0e-2
    twelve decades n = 130, 1024           4.0e-3   3.7e-3   7.4e-3   5.2e-3   1.2e-1   5.3e-2
obj(x0): 6.2e-2 (n = 7), <= 1.4e-2 otherwise.  2 of 7230 triples skipped (the sixth direction of the two warm SR1B + MoreThuenteB runs)."""
import functools

import numpy as np

import problems as P
import qn_replay as R
from qn_replay import EPS, LD, ld_matvec

KAPPA = 100.0
TB = 128
PLANS = [(3, 3), (1, 2, 3), (2, 2, 2)]   # H read after every call
WARM_PLANS = [(6,), (3, 3)]              # H read at the end only: replayed as one run of six from I
SIZES = [7, 130, 1000, 1020, 1024, 1152, 4096]


def c_g(n):
    return n + 4


def c_f(n):
    return 2 * n + 8


# ---- the problems ----
SOURCE = {}   # which matrix `synth` is: "oracle library" or "numpy"; the tests print it next to their ratios


def _oracle():
    """the oracle library, or None where it cannot exist (the package or a `make` is missing); a build that fails for another reason is an error"""
    try:
        from oracle import qn_oracle
        qn_oracle.build()
    except (ImportError, FileNotFoundError):
        SOURCE["synth"] = "numpy"
        return None
    SOURCE["synth"] = "oracle library"
    return qn_oracle


def _synth(n):
    diag = P.synth_diag(n, KAPPA)
    qo = _oracle()
    if qo is not None:
        q = np.array(qo.synth_rows(n, 0, n, P.SEED, diag), dtype=np.float64)
    else:
        rng = np.random.default_rng(P.SEED)
        u = rng.uniform(-1.0, 1.0, (n, n)) / n
        q = np.triu(u, 1) + np.triu(u, 1).T + np.diag(diag)
    b, x0 = P.synth_vectors(n)
    return q, b, x0


@functools.lru_cache(maxsize=None)
def problem(kind, n):
    """(q, b, x0), read-only"""
    q, b, x0 = _synth(n)
    if kind == "nonsym":
        rng = np.random.default_rng(n + 1)
        q = q + np.triu(rng.standard_normal((n, n)), 1) * (1e-3 / n)
    elif kind == "wide":
        rng = np.random.default_rng(n + 2)
        d = 10.0 ** rng.permutation(np.linspace(-3.0, 3.0, n))
        q = (q * d[:, None]) * d[None, :]
        q = np.triu(q) + np.triu(q, 1).T   # (the two roundings commute, but say so: symmetric bit for bit)
        b = b * d
    else:
        assert kind == "synth", kind
    q, b, x0 = np.ascontiguousarray(q), b.copy(), x0.copy()
    for v in (q, b, x0):
        v.setflags(write=False)
    return q, b, x0


def box(x0):
    """(lb, ub): a quarter of the entries clipped from below at x0, a quarter from above, a quarter free inside finite bounds, a quarter unbounded"""
    j = np.arange(x0.size) % 4
    lb = np.select([j == 0, j == 1, j == 2], [x0 + 0.5, x0 - 1.5, x0 - 1.0], -np.inf)
    ub = np.select([j == 0, j == 1, j == 2], [x0 + 1.5, x0 - 0.5, x0 + 1.0], np.inf)
    return lb, ub


# ---- truth and bounds ----
class Truth:
    def __init__(self, q, qabs, b, x):
        n = x.size
        xl, xa = x.astype(LD), np.abs(x)
        qx = ld_matvec(q, x)
        self.g = qx - b.astype(LD)
        self.f = np.dot(xl, qx) / 2 - np.dot(b.astype(LD), xl)
        gs = (qabs @ xa + np.abs(b)) * (1.0 + 1e-12)
        fs = (0.5 * float(xa @ (qabs @ xa)) + float(np.abs(b) @ xa)) * (1.0 + 1e-12)
        self.bg = 1.001 * c_g(n) * EPS * gs
        self.bf = 1.001 * c_f(n) * EPS * fs
        self.fscale = fs
        self.gnorm = float(np.sqrt(np.dot(self.g, self.g)))
        self.bgnorm = float(np.linalg.norm(self.bg))


class ClosureTruth:
    """the generic path: what the host closure returned IS the truth (bf = bg = 0)"""

    def __init__(self, f, g):
        self.f, self.g = LD(f), np.asarray(g, dtype=np.float64).astype(LD)
        self.bf, self.bg = 0.0, np.zeros(self.g.size)
        self.gnorm, self.bgnorm = float(np.sqrt(np.dot(self.g, self.g))), 0.0


_qabs = {}


def truth_factory(kind, n):
    """x -> Truth of the problem, cached by the bits of x (shared by every test of a process)"""
    q, b, _ = problem(kind, n)
    if (kind, n) not in _qabs:
        _qabs[(kind, n)] = (np.abs(q), {})
    qabs, cache = _qabs[(kind, n)]

    def truth(x):
        key = x.tobytes()
        if key not in cache:
            cache[key] = Truth(q, qabs, b, x)
        return cache[key]

    return truth


# ---- float64 restatements: three summation orders of a matrix-vector product and of an inner product ----
def _rsum(terms):
    """the last axis summed from the far end, one term at a time"""
    return np.add.accumulate(terms[..., ::-1], axis=-1)[..., -1]


def mv(order, m, v, mirrored=True, missing=None):
    """m @ v in float64.  "plain": numpy's; "reversed": every row from the far end; "blocked": 128 x 128 tiles of the upper block triangle, each
    off-diagonal tile adding its direct contribution to its block-row and (mirrored: from the same entries, as the symmetric half does) its
    transposed contribution to its block-column, per-block partial sums folded afterwards.  missing = (i, j), i < j in different blocks: the
    mirrored contribution m_ij v_i to entry j is left out (a planted fault)."""
    if order == "plain":
        return m @ v
    if order == "reversed":
        return _rsum(m * v)
    n = v.size
    nb = -(-n // TB)
    part = np.zeros((nb, n))      # part[J] holds what block-column / block-row J contributed to every entry
    for bi in range(nb):
        ri = slice(bi * TB, min(n, (bi + 1) * TB))
        for bj in range(bi, nb):
            rj = slice(bj * TB, min(n, (bj + 1) * TB))
            part[bj, ri] += m[ri, rj] @ v[rj]
            if bj > bi:
                tile = (m[ri, rj].T if mirrored else m[rj, ri])
                if missing is not None and ri.start <= missing[0] < ri.stop and rj.start <= missing[1] < rj.stop:
                    tile = tile.copy()
                    tile[missing[1] - rj.start, missing[0] - ri.start] = 0.0
                part[bi, rj] += tile @ v[ri]
    return part.sum(axis=0)


def dot(order, a, b):
    if order == "plain":
        return float(a @ b)
    if order == "reversed":
        return float(_rsum(a * b))
    return float(sum(float(a[i:i + TB] @ b[i:i + TB]) for i in range(0, a.size, TB)))


ORDERS = ("plain", "reversed", "blocked")


class RefSolver:
    """A float64 BFGS / DFP / SR1 run on a quadratic in the library's layout (trace records, xs[k] = x_{k+1}), free or in a box, continued over
    several calls, with the rank-2 form of the update and Armijo backtracking.  fault = (tag, ...) plants a defect:
      ("g_entry", k, rel)        the entry of largest |g| of the gradient the direction of iteration k is formed from is off by rel |g_j|
      ("drop_product", i, j, k)  Q_ij x_j missing from g_i at the accepted point of iteration k only (trial evaluations are right)
      ("mirror", i, j)           blocked order: the mirrored contribution of entry (i, j) missing from every evaluation
      ("f_off", rel)             f off by rel (1/2 |x|'|Q||x| + |b|'|x|)
      ("h_entry", k, i, j)       entries (i, j) and (j, i) of H left as they were by the update of iteration k
      ("no_mirror", i, j)        the returned H has its lower-triangle entry (i, j) from before the last update
      ("stale_dir", k)           the direction of iteration k formed without the latest update (the second of two pending ones dropped)
      ("stale_yu", k)            the update of iteration k takes its coefficients from the previous iteration's y'u
      ("project_dir",)           the projection applied to -H g instead of to x - H g
      ("sr1_den",)               SR1's denominator without the y'u term"""

    def __init__(self, q, b, x0, method, order="plain", box=None, fault=None, tol=1e-10):
        self.q, self.b, self.method, self.order, self.box, self.fault, self.tol = q, b, method, order, box, fault or ("none",), tol
        self.mirrored = bool(np.array_equal(q, q.T))
        self.x = np.array(x0, dtype=np.float64) if box is None else np.clip(x0, box[0], box[1])
        self.x0p = self.x.copy()
        self.n = self.x.size
        self.h = np.eye(self.n)
        self.h_before = self.h.copy()
        self.k, self.tr, self.xs = 0, [], []
        self.f, self.g = self.ev(self.x)
        self.yu_prev = None

    def ev(self, x, accepted=False):
        ft = self.fault
        qx = mv(self.order, self.q, x, self.mirrored, missing=ft[1:] if ft[0] == "mirror" else None)
        g = qx - self.b
        f = 0.5 * dot(self.order, x, qx) - dot(self.order, self.b, x)
        if ft[0] == "drop_product" and accepted and ft[3] == self.k:
            g[ft[1]] = (qx[ft[1]] - self.q[ft[1], ft[2]] * x[ft[2]]) - self.b[ft[1]]
        if ft[0] == "f_off":
            xa = np.abs(x)
            f += ft[1] * (0.5 * float(xa @ (np.abs(self.q) @ xa)) + float(np.abs(self.b) @ xa))
        return f, g

    def advance(self, iters):
        ft = self.fault
        for _ in range(iters):
            x, f, g, k = self.x, self.f, self.g, self.k
            gd = g.copy()
            if ft[0] == "g_entry" and ft[1] == k:
                j = int(np.argmax(np.abs(gd)))
                gd[j] += ft[2] * abs(gd[j])
            hd = self.h_before if (ft[0] == "stale_dir" and ft[1] == k) else self.h
            hg = mv(self.order, hd, gd)
            if self.box is None:
                d = -hg
            elif ft[0] == "project_dir":
                d = np.clip(-hg, self.box[0], self.box[1])
            else:
                d = np.clip(x - hg, self.box[0], self.box[1]) - x
            gd0, t, evals = float(g @ d), 1.0, 0
            for _ in range(60):
                ftrial, _g = self.ev(x + t * d)
                evals += 1
                if np.isfinite(ftrial) and ftrial - f <= 1e-4 * t * gd0:
                    break
                t *= 0.5
            xn = x + t * d
            fn, gn = self.ev(xn, accepted=True)
            s, y = xn - x, gn - g
            self.tr.append(dict(f=f, gnorm=float(np.sqrt(g @ g)), t=t, s_norm=float(np.sqrt(s @ s)), y_norm=float(np.sqrt(y @ y)), updated=1,
                                n_evals=evals + 1))
            self.xs.append(xn)
            u = mv(self.order, self.h, y)
            ys, yu = dot(self.order, s, y), dot(self.order, y, u)
            yu_used = self.yu_prev if (ft[0] == "stale_yu" and ft[1] == k and self.yu_prev is not None) else yu
            if self.method == "sr1" and ft[0] == "sr1_den":
                css = 1.0 / ys
                csu, cuu = -css, css
            else:
                css, csu, cuu = R.coefficients(self.method, ys, yu_used)
            self.yu_prev = yu
            self.h_before = self.h
            self.h = self.h + css * np.outer(s, s) + csu * (np.outer(s, u) + np.outer(u, s)) + cuu * np.outer(u, u)
            if ft[0] == "h_entry" and ft[1] == k:
                i, j = ft[2], ft[3]
                self.h[i, j], self.h[j, i] = self.h_before[i, j], self.h_before[j, i]
            self.x, self.f, self.g, self.k = xn, fn, gn, k + 1

    def records(self):
        return list(self.tr), np.array(self.xs)

    def start(self):
        """the point the run started from (a bounded solver projects x0)"""
        return self.x0p

    def inv_hessian(self):
        h = self.h.copy()
        if self.fault[0] == "no_mirror":
            i, j = self.fault[1:]
            h[i, j] = self.h_before[i, j]
        return h


# ---- a run cut into segments, and its replay ----
def run_plan(runner, x_start, plan, read_h=True):
    """Drive `runner` (advance(k), records(), inv_hessian()) through the calls of `plan` -> the segments to replay, dicts of x0, h0, tr, xs, h_end.
    read_h: one segment per call, each from the matrix read after the call before; otherwise the whole plan as one segment from I."""
    segs, done, x, h = [], 0, np.array(x_start, dtype=np.float64), None
    for iters in plan:
        runner.advance(iters)
        tr, xs = runner.records()
        if read_h:
            assert len(tr) >= done + 1, ("the call left no record", len(tr), done)
            h_end = runner.inv_hessian()
            segs.append(dict(x0=x, h0=h, tr=tr[done:], xs=xs[done:len(tr)], h_end=h_end))
            done, x, h = len(tr), np.array(xs[len(tr) - 1]), h_end
    if not read_h:
        tr, xs = runner.records()
        segs.append(dict(x0=x, h0=None, tr=tr, xs=xs[:len(tr)], h_end=runner.inv_hessian()))
    return segs


def replay_plan(name, truth, method, segs, box=None, symmetric=False):
    """one Report per segment; every iteration of a segment is replayed (segments here are at most six iterations long)"""
    return [R.replay(f"{name}/seg{i}", truth, sg["x0"], method, sg["tr"], sg["xs"], h0=sg["h0"], box=box, h_dev=sg["h_end"], symmetric=symmetric,
                     iters=len(sg["tr"]), kind="quad") for i, sg in enumerate(segs)]
