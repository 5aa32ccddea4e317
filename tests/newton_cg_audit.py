"""Audit of every NewtonCG direction of a whole run in extended precision (tests/test_ref_newton_cg_audit.py applies it to the float64 restatement and
plants the faults it has to reject, tests/test_gpu_newton_cg_audit.py applies it to the GPU).  Test infrastructure: the product does not import this.

A RECORDED RUN holds, per outer iteration k: x_k, the float64 g_k the direction was built from BIT FOR BIT (with the true gradient as right-hand side
the distances below grow to 3e-8 at the last iterations: g carries ulps of cancelled terms), d_k, t_k, x_{k+1}, the inner count j_k, the
negative-curvature and fallback counters before and after, and for Jacobi the run's own 1 / M of that iteration.  Every direction is checked ON ITS OWN
from these; nothing accumulates from one iteration to the next.  The product v -> H(x) v is each kind's np.longdouble truth (`LseOps`,
`LogisticOps`, `MultinomialOps` below: the formulas of lse_hess_vec_cases, ref_logistic, ref_multinomial on the problem data, a sparse kind through
its densified matrix -- an absent entry is an exact zero), never the device's association.

(a) BOOKKEEPING, every direction.  x_{k+1} = fl(x_k + fl(t_k d_k)) bit for bit.  A negative-curvature count that rose with j_k = 0, or a fallback
    count that rose, means d_k = -g_k bit for bit; otherwise g_k.d_k < 0 (longdouble).  Counters never fall.  A violated equality is the ratio inf.

(b) THE INEXACT-NEWTON CONTRACT, every direction that ended by the tolerance (1 <= j_k < cap, no negative-curvature rise, no fallback).  With
    z = -d_k and eta_k = min(eta_max, ||g_k||^(1/2)), in longdouble:      ||g_k - H(x_k) z||_2 <= eta_k ||g_k||_2 + slack_k.
    slack_k is the drift between the true residual and the recurrence residual r^ the device tested.  The device computes, per inner step,
        z^' = fl(z^ + fl(alpha p)),   r^' = fl(r^ - fl(alpha q^)),   q^ = H p + dq,  |dq| <= E(p) (the kind's derived product bound at p).
    With e = (g - H z^) - r^:  e' = e - H dz + alpha dq - dr, where dz and dr are the two roundings of each update:
        |dz| <= u (|alpha p| + |z^'|),   |dr| <= u (|alpha q^| + |r^'|),   |H dz| <= S |dz| entrywise (S: the kind's scale matrix, |H| <= S).
    e_0 = 0 (r^_0 = g exactly), so  |e_j| <= sum over the j steps of  S (u (|alpha p| + |z^'|)) + alpha E(p) + u (|alpha q^| + |r^'|)  entrywise,
    and slack_k is the 2-norm of that sum.  The magnitudes are those of the float64 stand-in "numpy" of (c) -- the device's own differ from them
    in second order --, and u is taken as EPS = 2^-52, twice the unit roundoff: the factor of two pays for the second-order terms and for
    evaluating the bound itself in floating point (sums of non-negative terms).  THE TEST's own roundings: rr' = r^.r^ and gg = g.g are n-term sums
    of non-negative products, relative error (n + 1) u each in any order; sqrt halves it and adds u; sqrt(sqrt(gg)) once more; the product
    eta sqrt(gg) adds u: together below (2 n + 8) u of eta ||g||, added to the slack.  Nothing here is measured on a device.

(c) THE ITERATE, where float64 can tell (1 <= j_k, no negative-curvature rise, no fallback: H(x_k) is then positive along everything used).  From
    (x_k, g_k) and the run's own 1 / M the rules of ref_newton_cg.py / ref_newton_pcg.py are run for exactly j_k steps in longdouble, and in four
    float64 STAND-INS: "numpy" (numpy's products), "reversed" (every sum over flipped operands), "moved" (numpy's, every product moved by
    newton_cg_cases.PRODUCT_UNITS units of 2^-53 S |v| with random signs, seed 1) and "aligned" (the same units, every entry moved in the
    direction of v_j: the largest shift of kappa = v.Hv the units allow.  The random signs of "moved" cancel like a random walk; at j_k = 1 the
    whole distance is that one scalar, and one draw can fall a hundred times below another -- the moved RUNS of the CPU test, seed 2 on
    (5, 2050), met exactly this against seed 1).  e_s = ||z_s - z_ext||_H / ||z_ext||_H is each stand-in's energy distance
    (H = H(x_k) in longdouble).  The direction is LICENSED when MARGIN max_s e_s <= LICENCE = 1e-9, the tolerance the suite already has, and then
    the audited z = -d_k must satisfy ||z - z_ext||_H / ||z_ext||_H <= MARGIN max_s e_s.  On badly scaled problems float64 CG loses orthogonality
    after tens of steps and the stand-ins part ways from the extended iterate (0.59 without, 0.065 with Jacobi): those directions are not
    licensed, and (a), (b) still hold them.
    A distance below FLOOR = 2^-52 says nothing about an order -- z is stored in float64, its last rounding alone moves it by up to u per entry,
    and at j_k = 1 (z = alpha g, one scalar) two stand-ins often land on the same bits --, so max_s e_s is floored there.
    MARGIN is measured on the CPU, never on a device (tests/test_ref_newton_cg_audit.py::test_margin_is_measured): one ORDER stand-in at a time
    ("numpy", "reversed") is held out over every direction of every CPU case, and the largest ratio of its distance to the (floored) maximum of
    the others is taken -- the device's summation order is a further order that no stand-in has.  "moved" and "aligned" are not held out: they
    are envelopes, deliberately four units of a worst-case bound where a real order spends a fraction of one, and sit far above the two orders
    (1.5e4 times at the most); holding them out would measure the envelope's height, not what an unseen order can add, and would only widen
    MARGIN.  MEASURED: largest held-out ratio 12.62 (log-sum-exp (5, 2050) under StrongWolfe, the fsum-order run, a direction of one inner
    step: the reversed order against the rest); MARGIN = twice that, rounded up, at least 4 = 26.

(d) THE STOPPING STEP, licensed directions that ended by the tolerance.  The extended loop's ||r_j|| must satisfy ||r|| <= eta ||g|| at step j_k
    (ratio ||r_j|| / (eta ||g||) <= 1) and must not at step j_k - 1 (ratio eta ||g|| / ||r_(j-1)|| < 1).  A step whose extended ||r|| lies
    within relative TIE = 1e-10 of eta ||g|| is a tie: skipped and counted.
"""
import math
import zlib

import numpy as np

import lse_hess_vec_cases as HV
import newton_cg_cases as NC
import ref_logistic as RL
import ref_multinomial as RM
import ref_newton_pcg as RP

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 ** -52
INF = float("inf")
LICENCE = 1e-9
TIE = 1e-10
FLOOR = EPS
MARGIN = 26.0
STAND_INS = ("numpy", "reversed", "moved", "aligned")
ORDER_STAND_INS = ("numpy", "reversed")
MOVED_SEED = 1
PRODUCT_UNITS = NC.PRODUCT_UNITS
_UP = 1.0 + 2.0 ** -20  # the bounds are sums of non-negative float64 terms: their own rounding, with room


def _flip(mat):
    return np.ascontiguousarray(mat[:, ::-1])


def _mv(mat, flipped, vec, order):
    """mat @ vec; "reversed": every row's sum over the flipped operands -- another summation order of the same terms"""
    return mat @ vec if order == "numpy" else flipped @ np.ascontiguousarray(vec[::-1])


def _dot64(order):
    if order == "reversed":
        return lambda a, b: float(np.dot(a[::-1], b[::-1]))
    return lambda a, b: float(np.dot(a, b))


def _ld_dot(a, b):
    return (a * b).sum()


def _moved(q, v, scale, seed=MOVED_SEED):
    rng = np.random.default_rng(zlib.crc32(np.ascontiguousarray(v).tobytes()) ^ seed)
    return q + PRODUCT_UNITS * U * rng.uniform(-1.0, 1.0, q.size) * scale


# ---- the kinds: v -> H(x) v in longdouble (the truth), in float64 (the stand-ins), the scale matrix S >= |H| and the product's derived bound ----
class _Point:
    """one kind at one x.  hv_ld(v): longdouble truth; hv64(v, stand_in): float64; scale(w): S w for w >= 0; bound(v): E(v) >= |float64 H v - H v|"""

    def hv64(self, v, stand_in):
        if stand_in == "moved":
            return _moved(self._hv64(v, "numpy"), v, self.scale(np.abs(v)))
        if stand_in == "aligned":
            return self._hv64(v, "numpy") + PRODUCT_UNITS * U * np.where(v < 0.0, -1.0, 1.0) * self.scale(np.abs(v))
        return self._hv64(v, stand_in)


class LseOps:
    """f = log sum exp(A x + c) + mu/2 ||x||^2 (lse_hess_vec_cases: H v = A'(p o (A v)) - gbar (p . (A v)) + mu v)"""

    def __init__(self, a, c, mu):
        self.a, self.c, self.mu = a, c, mu
        self.at_, self.af, self.atf = np.ascontiguousarray(a.T), _flip(a), _flip(np.ascontiguousarray(a.T))
        self.aa = np.abs(a)
        self.n = a.shape[1]

    def at(self, x):
        return _LsePoint(self, x)


class _LsePoint(_Point):
    def __init__(self, o, x):
        self.o = o
        self.al, self.p, self.gbar = HV.weights(o.a, o.c, x)
        self.w64 = {}
        for order in ("numpy", "reversed"):
            z = _mv(o.a, o.af, x, order) + o.c
            e = np.exp(z - z.max())
            p = e / (e.sum() if order == "numpy" else e[::-1].sum())
            self.w64[order] = (p, _mv(o.at_, o.atf, p, order))
        m, n = o.a.shape
        self.p64 = self.p.astype(np.float64)
        self.g_abs = o.aa.T @ self.p64
        live = np.isfinite(o.c)
        zcap = float(np.max(o.aa[live] @ np.abs(x) + np.abs(o.c[live])))
        b = (2 * m + 4 * (n + 1) * zcap + 16) * U  # lse_hess_vec_cases: B, and B_v = 2 B + (n + 4) u
        self.bv = (2.0 * b + (n + 4) * U) * (1.0 + 2.0 ** -11)

    def hv_ld(self, v):
        w = self.p * (self.al @ v)
        return self.al.T @ w - self.gbar * w.sum() + LD(self.o.mu) * v

    def _hv64(self, v, order):
        o = self.o
        p, gbar = self.w64[order]
        w = p * _mv(o.a, o.af, v, order)
        ubar = float(np.sum(w)) if order == "numpy" else float(np.sum(w[::-1]))
        return (_mv(o.at_, o.atf, w, order) - ubar * gbar) + o.mu * v

    def scale(self, w):
        o = self.o
        return (o.aa.T @ (self.p64 * (o.aa @ w)) + self.g_abs * float(self.g_abs @ w) + abs(o.mu) * w) * _UP

    def bound(self, v):
        return self.bv * self.scale(np.abs(v))


class LogisticOps:
    """f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2 (ref_logistic: H v = A'(d o (A v)) + mu v); a sparse A through its densified matrix"""

    def __init__(self, a, y, w, mu):
        self.a, self.y, self.w, self.mu = a, y, np.ones(a.shape[0]) if w is None else w, mu
        self.at_, self.af, self.atf = np.ascontiguousarray(a.T), _flip(a), _flip(np.ascontiguousarray(a.T))
        self.aa, self.al = np.abs(a), a.astype(LD)
        self.n = a.shape[1]
        self.yw = np.asarray(y, dtype=np.float64) * self.w

    def at(self, x):
        return _LogisticPoint(self, x)


class _LogisticPoint(_Point):
    def __init__(self, o, x):
        self.o = o
        truth = RL.truth_and_bound(o.a, o.y, o.w, o.mu, x)
        self.d = truth["d"]
        self.d64 = {order: RL.row_terms(o.yw, _mv(o.a, o.af, x, order))[2] for order in ("numpy", "reversed")}
        self.dmag, self.bd = self.d.astype(np.float64), truth["bd"].astype(np.float64)
        m, n = o.a.shape
        self.c1 = RL.gamma(n + 1) + RL.gamma(m + 2) + U

    def hv_ld(self, v):
        return self.o.al.T @ (self.d * (self.o.al @ v)) + LD(self.o.mu) * v

    def _hv64(self, v, order):
        o = self.o
        return _mv(o.at_, o.atf, self.d64[order] * _mv(o.a, o.af, v, order), order) + o.mu * v

    def scale(self, w):
        o = self.o
        return (o.aa.T @ (self.dmag * (o.aa @ w)) + abs(o.mu) * w) * _UP

    def bound(self, v):  # ref_logistic's |q_j - q*_j|, the reference's share included
        o = self.o
        av = np.abs(v)
        uk = o.aa @ av
        return (o.aa.T @ (self.bd * uk + self.c1 * (self.dmag * uk)) + 3 * U * abs(o.mu) * av) * RL.REF * _UP


class MultinomialOps:
    """softmax regression, class-major x (ref_multinomial: (H v)_k = sum_r t_rk a_r + mu V_k); a sparse A through its densified matrix"""

    def __init__(self, a, y, w, k, mu):
        self.a, self.y, self.k, self.mu = a, np.asarray(y).astype(np.int64), k, mu
        self.w = np.ones(a.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
        self.af, self.aa, self.al, self.wl = _flip(a), np.abs(a), a.astype(LD), self.w.astype(LD)
        self.n = k * a.shape[1]

    def at(self, x):
        return _MultinomialPoint(self, x)


class _MultinomialPoint(_Point):
    def __init__(self, o, x):
        self.o, self.x = o, x
        self.p = RM.truth_and_bound(o.a, o.y, o.w, o.k, o.mu, x)["p"]
        nf = o.a.shape[1]
        self.p64 = {"numpy": RM.probabilities_f64(o.a, o.y, o.w, o.k, x),
                    "reversed": RM.row_terms(o.af @ np.ascontiguousarray(x.reshape(o.k, nf).T[::-1]), o.y, o.w)[2]}
        self.pmag = self.p.astype(np.float64)

    def hv_ld(self, v):
        o = self.o
        vm = v.reshape(o.k, -1)
        u = o.al @ vm.T
        ub = np.sum(self.p * u, axis=1)
        t = np.where((o.w != 0.0)[:, None], (o.wl[:, None] * self.p) * (u - ub[:, None]), LD(0))
        return (t.T @ o.al + LD(o.mu) * vm).ravel()

    def _hv64(self, v, order):
        o = self.o
        p = self.p64[order]
        vm = v.reshape(o.k, -1)
        rev = order == "reversed"
        u = o.af @ np.ascontiguousarray(vm.T[::-1]) if rev else o.a @ vm.T
        ub = np.zeros(o.a.shape[0])
        for j in (range(o.k - 1, -1, -1) if rev else range(o.k)):
            ub = ub + p[:, j] * u[:, j]
        t = np.where((o.w != 0.0)[:, None], (o.w[:, None] * p) * (u - ub[:, None]), 0.0)
        back = (np.ascontiguousarray(t.T[:, ::-1]) @ np.ascontiguousarray(o.a[::-1])) if rev else t.T @ o.a
        return (back + o.mu * vm).ravel()

    def scale(self, w):  # multinomial_cases.moved_product's scale
        o = self.o
        au = o.aa @ w.reshape(o.k, -1).T
        return (((o.w[:, None] * self.pmag * (au + np.sum(self.pmag * au, axis=1)[:, None])).T @ o.aa).ravel() + abs(o.mu) * w) * _UP

    def bound(self, v):  # ref_multinomial's own |q_kj - q*_kj| at v
        o = self.o
        return RM.truth_and_bound(o.a, o.y, o.w, o.k, o.mu, self.x, v)["bq"].astype(np.float64) * _UP


# ---- the recorded run ----
class Direction:
    __slots__ = ("x", "g", "d", "t", "x_next", "j", "neg0", "neg1", "fb0", "fb1", "minv")

    def __init__(self, x, g, d, t, x_next, j, neg0, neg1, fb0, fb1, minv=None):
        self.x, self.g, self.d, self.x_next = (np.array(v, dtype=np.float64) for v in (x, g, d, x_next))
        self.t, self.j, self.neg0, self.neg1, self.fb0, self.fb1 = float(t), int(j), int(neg0), int(neg1), int(fb0), int(fb1)
        self.minv = None if minv is None else np.array(minv, dtype=np.float64)


class Run:
    def __init__(self, ops, cap, eta_max=0.5, jacobi=False, name=""):
        self.ops, self.cap, self.eta_max, self.jacobi, self.name, self.dirs = ops, int(cap), eta_max, jacobi, name, []


class _Recording:
    """mixed in front of ref_newton_cg.NewtonCG / ref_newton_pcg.JacobiNewtonCG: keeps what a recorded run holds, changes nothing"""

    def compute_direction(self, eval_x_k):
        rec = dict(x=self.x.copy(), g=np.array(eval_x_k[1], dtype=np.float64), neg0=self.neg_curv, fb0=self.fallbacks)
        d = super().compute_direction(eval_x_k)
        rec.update(d=np.array(d), j=self.inner[-1], neg1=self.neg_curv, fb1=self.fallbacks, minv=self.minv_used(rec["x"]))
        self._rec = rec
        return d

    def minv_used(self, x):
        if not hasattr(self, "diag_at"):
            return None
        minv = RP.minv_of(self.diag_at(x))[0]
        return minv * minv if getattr(self, "twice", False) else minv

    def update_next_iterate(self, line_search, eval_x_k, oracle, direction, max_iter_line_search):
        t = super().update_next_iterate(line_search, eval_x_k, oracle, direction, max_iter_line_search)
        self.records.append(Direction(t=t, x_next=self.x.copy(), **self._rec))
        return t


_recording_classes = {}


def adopt(solver):
    """make a restatement solver (as a case module's run_ref built it, before its first iteration) record its run; the same object is returned"""
    base = solver.__class__
    if base not in _recording_classes:
        _recording_classes[base] = type("Recording" + base.__name__, (_Recording, base), {})
    solver.__class__ = _recording_classes[base]
    solver.records = []
    return solver


def run_of(solver, ops, name=""):
    run = Run(ops, solver.cap, solver.eta_max, hasattr(solver, "diag_at"), name)
    run.dirs = list(solver.records)
    return run


# ---- the rules, for exactly `steps` inner steps, in any arithmetic ----
def cg_steps(g, hv, minv, steps, dot, on_step=None):
    """(z, [||r_0||, ..., ||r_steps||]) by rules 2 to 7 (2', 5', 7' with a minv), the loop's own exits ignored; None where a curvature is not
    positive and finite (rule 4 would have ended the loop)"""
    z, r = g * 0, g.copy()
    p = g.copy() if minv is None else minv * g
    rho = dot(r, r) if minv is None else dot(r, minv * r)
    norms = [np.sqrt(dot(g, g))]
    for i in range(steps):
        q = hv(p)
        kappa = dot(p, q)
        if not (kappa > 0) or not np.isfinite(kappa):
            return None
        alpha = rho / kappa
        ap, aq = alpha * p, alpha * q
        z, r = z + ap, r - aq
        rr = dot(r, r)
        norms.append(np.sqrt(rr))
        if on_step is not None:
            on_step(alpha, p, ap, aq, z, r)
        if i + 1 == steps:
            break
        if not (rho > 0):
            return None
        if minv is None:
            beta, rho = rr / rho, rr
            p = r + beta * p
        else:
            y = minv * r
            rz = dot(r, y)
            beta, rho = rz / rho, rz
            p = y + beta * p
    return z, norms


def _energy(pt, e, zx):
    """||e||_H / ||zx||_H in longdouble"""
    num, den = _ld_dot(e, pt.hv_ld(e)), _ld_dot(zx, pt.hv_ld(zx))
    if not (den > 0) or not (num >= 0):
        return INF
    return float(np.sqrt(num / den))


def audit_direction(run, k, margin=MARGIN):
    """every check of direction k: dict(k, j, ended, licensed, tie, e (the stand-ins' distances), ratios a, b, c, d_late, d_early -- None where the
    check does not apply --, inside_b: ||g - H z|| / (eta ||g||) without the slack, slack_share: slack / (eta ||g||))"""
    dr, ops = run.dirs[k], run.ops
    out = dict(k=k, j=dr.j, licensed=False, tie=False, e={}, a=0.0, b=None, c=None, d_late=None, d_early=None, inside_b=None, slack_share=None, dist=None)
    neg_rose, fb_rose = dr.neg1 > dr.neg0, dr.fb1 > dr.fb0
    # (a)
    bad = dr.x_next.tobytes() != (dr.x + dr.t * dr.d).tobytes() or dr.neg1 < dr.neg0 or dr.fb1 < dr.fb0
    if (neg_rose and dr.j == 0) or fb_rose:
        bad = bad or dr.d.tobytes() != (-dr.g).tobytes()
    else:
        bad = bad or not (_ld_dot(dr.g.astype(LD), dr.d.astype(LD)) < 0)
    if k > 0:
        bad = bad or dr.neg0 < run.dirs[k - 1].neg1 or dr.fb0 < run.dirs[k - 1].fb1
    out["a"] = INF if bad else 0.0
    out["ended"] = "fallback" if fb_rose else "negcurv" if neg_rose else "cap" if dr.j >= run.cap else "tol"
    if dr.j < 1 or neg_rose:
        return out
    pt = ops.at(dr.x)
    gl, zl = dr.g.astype(LD), (-dr.d).astype(LD)
    gnorm = np.sqrt(_ld_dot(gl, gl))
    eta = min(LD(run.eta_max), np.sqrt(gnorm))
    minv = dr.minv if run.jacobi else None
    # the stand-ins; "numpy" also sums the drift of (b)
    drift = np.zeros(dr.g.size)

    def on_step(alpha, p, ap, aq, z, r):
        drift[:] += pt.scale(EPS * (np.abs(ap) + np.abs(z))) + abs(alpha) * pt.bound(p) + EPS * (np.abs(aq) + np.abs(r))
    ext = cg_steps(gl, pt.hv_ld, None if minv is None else minv.astype(LD), dr.j, _ld_dot)
    stand = {}
    for s in STAND_INS:
        stand[s] = cg_steps(dr.g, lambda v, s=s: pt.hv64(v, s), minv, dr.j, _dot64(s), on_step if s == "numpy" else None)
    # (b)
    if out["ended"] == "tol":
        resid = gl - pt.hv_ld(zl)
        rnorm = np.sqrt(_ld_dot(resid, resid))
        slack = float(np.linalg.norm(drift)) * _UP + (2 * dr.g.size + 8) * U * float(eta * gnorm) if stand["numpy"] is not None else INF
        out["inside_b"] = float(rnorm / (eta * gnorm))
        out["slack_share"] = float(slack / float(eta * gnorm))
        out["b"] = float(rnorm / (eta * gnorm + LD(slack)))
    # (c): the licence is the direction's (x_k, g_k, j_k), whatever d_k is; the distance is asserted where d_k = -z
    if ext is None:
        return out
    zx, norms = ext
    for s in STAND_INS:
        out["e"][s] = INF if stand[s] is None else _energy(pt, stand[s][0].astype(LD) - zx, zx)
    emax = max(max(out["e"].values()), FLOOR)
    out["licensed"] = bool(margin * emax <= LICENCE)
    if fb_rose:
        return out
    out["dist"] = _energy(pt, zl - zx, zx)
    if not out["licensed"]:
        return out
    out["c"] = out["dist"] / (margin * emax)
    # (d)
    if out["ended"] == "tol":
        bound = eta * gnorm
        late, early = float(norms[dr.j] / bound), float(bound / norms[dr.j - 1])
        if abs(late - 1.0) <= TIE or abs(early - 1.0) <= TIE:
            out["tie"] = True
        else:
            out["d_late"], out["d_early"] = late, early
    return out


CHECKS = ("a", "b", "c", "d_late", "d_early")


def audit(run, margin=MARGIN):
    """every direction of a recorded run: dict(rows, directions, with_steps (j >= 1), licensed, ties, worst (per check), inside_b (the largest
    ||g - H z|| / (eta ||g||) of a tolerance exit), failures [(k, check, ratio)])"""
    rows = [audit_direction(run, k, margin) for k in range(len(run.dirs))]
    worst = {c: max([r[c] for r in rows if r[c] is not None], default=0.0) for c in CHECKS}
    fails = [(r["k"], c, r[c]) for r in rows for c in CHECKS if r[c] is not None and (r[c] >= 1.0 if c == "d_early" else r[c] > 1.0)]
    return dict(rows=rows, name=run.name, directions=len(rows), with_steps=sum(1 for r in rows if r["j"] >= 1 and r["ended"] in ("tol", "cap")),
                licensed=sum(1 for r in rows if r["licensed"]), ties=sum(1 for r in rows if r["tie"]), worst=worst,
                inside_b=max([r["inside_b"] for r in rows if r["inside_b"] is not None], default=0.0),
                slack_share=max([r["slack_share"] for r in rows if r["slack_share"] is not None], default=0.0), failures=fails)


def line(rep):
    w = rep["worst"]
    return (f"{rep['name']}: directions {rep['directions']}, with inner steps {rep['with_steps']}, licensed {rep['licensed']}, ties {rep['ties']}; worst "
            f"a {w['a']:.3g}  b {w['b']:.4f} (without slack {rep['inside_b']:.4f}, slack share {rep['slack_share']:.1e})  c {w['c']:.3g}  "
            f"d late {w['d_late']:.4f} early {w['d_early']:.4f}")


def held_out_ratio(rep):
    """(the largest e_s / max(the other stand-ins' e, FLOOR) over the directions of a report with an ORDER stand-in held out -- MARGIN's measurement --,
    the same with "moved" held out, for the record); directions where a stand-in broke down are left out"""
    worst = {"orders": 0.0, "moved": 0.0}
    for r in rep["rows"]:
        e = r["e"]
        if len(e) < len(STAND_INS) or not all(math.isfinite(v) for v in e.values()):
            continue
        for s in STAND_INS:
            key = "orders" if s in ORDER_STAND_INS else "moved"
            worst[key] = max(worst[key], e[s] / max(max(v for t, v in e.items() if t != s), FLOOR))
    return worst["orders"], worst["moved"]


# ---- the cases both test files audit: (family, ...) -> the kind's operations, and the restatement's recorded run ----
import logistic_cases as LC  # noqa: E402
import multinomial_cases as MC  # noqa: E402
import precond_cases as PC  # noqa: E402
import sparse_logistic_cases as SL  # noqa: E402
import sparse_multinomial_cases as SM  # noqa: E402

LSE_CASES = [("lse", m, n, ls) for (m, n, ls) in NC.CASES]
# shapes of each other kind with and without a padded n (65 = 13 * 5: n_pad 80), BackTracking and StrongWolfe.  Dense logistic (96, 64) under StrongWolfe
# has one direction of 18 inner steps whose "moved" stand-in sits at 9e-11 of the extended iterate -- not licensed at MARGIN --, so (257, 200) carries
# that search there (every direction licensed, the worst stand-in at 1.3e-11)
UNSCALED_CASES = ([("logistic", 96, 64, "bt"), ("logistic", 257, 200, "wolfe"), ("logistic", 40, 65, "bt"), ("logistic", 40, 65, "wolfe")]
                  + [("slogistic", m, n, ls) for (m, n) in [(96, 64), (40, 65)] for ls in NC.SEARCHES]
                  + [("multinomial", m, n, k, ls) for (m, n, k) in [(96, 16, 4), (40, 13, 5)] for ls in NC.SEARCHES]
                  + [("smultinomial", m, n, k, ls) for (m, n, k) in [(96, 16, 4), (40, 13, 5)] for ls in NC.SEARCHES])
PRECOND_PROBLEMS = list(PC.CASES) + [(kind,) + PC.COUNTER + ("bt",) for kind in PC.KINDS]
PRECOND_CASES = [("precond",) + p + (pc,) for p in PRECOND_PROBLEMS for pc in ("none", "jacobi")]
_ops = {}


def ops_of(case):
    fam = case[0]
    key = case[:-1] if fam != "precond" else case[:4]
    if key not in _ops:
        if fam == "lse":
            a, c, mu, _ = NC.problem(case[1], case[2])
            _ops[key] = LseOps(a, c, mu)
        elif fam == "logistic":
            a, y, w, mu, _, _ = LC.problem(case[1], case[2])
            _ops[key] = LogisticOps(a, y, w, mu)
        elif fam == "slogistic":
            pr = SL.problem(case[1], case[2])
            _ops[key] = LogisticOps(pr["a"], pr["y"], pr["w"], pr["mu"])
        elif fam == "multinomial":
            a, y, w, k, mu, _, _ = MC.problem(*case[1:4])
            _ops[key] = MultinomialOps(a, y, w, k, mu)
        elif fam == "smultinomial":
            pr = SM.problem(*case[1:4])
            _ops[key] = MultinomialOps(pr["a"], pr["y"], pr["w"], pr["k"], pr["mu"])
        else:
            pr = PC.problem(case[2], case[3], case[1])
            _ops[key] = LogisticOps(pr["a"], pr["y"], pr["w"], pr["mu"])
    return _ops[key]


def _run_ref(case, **kw):
    fam = case[0]
    if fam == "precond":
        return PC.run_ref(case[1], case[2], case[3], case[4], case[5], **kw)
    mod = {"lse": NC, "logistic": LC, "slogistic": SL, "multinomial": MC, "smultinomial": SM}[fam]
    return mod.run_ref(*case[1:], **kw)


def ref_run(case, order="numpy", seed=None, solver_class=None, prepare=None, **kw):
    """the restatement's whole run on one case, recorded: (Run, solver, status).  solver_class: a subclass to run in its place, prepare(solver): its
    settings (the planted faults)"""
    s = _run_ref(case, iters=0, order=order, seed=seed, **kw)[0]
    if solver_class is not None:
        s.__class__ = solver_class
    if prepare is not None:
        prepare(s)
    adopt(s)
    _, _, status = _run_ref(case, order=order, seed=seed, solver=s, **kw)
    return run_of(s, ops_of(case), f"{case} {order}{'' if seed is None else ' moved ' + str(seed)}"), s, status
