"""The cases of the step-by-step replay of SPG, projected gradient and the projected Newton pair (tests/vec_replay.py), chosen for the edges of
csrc/qn_vec.hip.h; tests/test_ref_vec_replay.py licenses every one on the float64 restatements in three summation orders (no skipped
iteration, no undecidable decision), tests/test_gpu_vec_replay.py runs them on the GPU.

Sizes: 1, 2, 5, 6 (QN_SMALL_N and its neighbour); 7, 15, 16, 17 (n_pad is a multiple of 16); 2047, 2048, 2049 (one workgroup against two);
4099 (three, the last ragged); 2^19 + 2051 (G = 258: threads 0 and 1 of vec_sum_parts fold two shares each); 2^21 + 3 (G = 1024, more than
four trips of the grid-stride loop, three iterations).  The Newton pair: 1, 2, 5, 6, 7, 15, 16, 17, 130, with all three searches.

Problems: "spd" a seeded SPD quadratic of kappa = 100 (H = R D R, R a Householder reflection, applied in O(n); dense up to n = 130, where
the Newton pair reads it; `scale` multiplies D, so that with_lambdas(0.5, 2.0) clamps on both sides at scale 3); "quartic" the same plus
sum x^4 / 4 (Newton needs more than one step); "chain" the double-well chain of spg_cases.chain_fn (non-convex: from 0.2 x0 the first steps
have s.y < 0, and f rises over the fourth, which the call plans make their boundary); "crafted" a separable quadratic on dyadic numbers with,
by j mod 8, entries on lb pushed outward, on lb pushed inward, the same on ub, entries that REACH lb / ub with the first step and are pushed
inward there, entries with one infinite bound and entries with none -- these creep towards +-0.75 and cross the line search's own bound
+-0.4375 with the fourth step, so BackTrackingB's "moved" is false, then true; "crossing" every entry crosses the search's bound with the
first step and c1 = 0.6 makes that decision depend on diff2; "huber" pseudo-Huber with a tiny delta under lambda >= 50: interpolated steps
are rejected down to t <= 0.1 (GLLQuadratic's `halve`); "walled" spd with f = inf beyond a radius; "sep" a cheap separable convex function
for the large sizes; "tri" the device SparseQuadratic of sparse_cases.tri (only d_k, gnorm, x_{k+1} and the update scalars apply: the trial
values are not visible from outside).  GLL m = 1, 3, 10 and, at n = 7 over 70 iterations, 64 (QN_GLL_MAX_M).  THE RING'S LENGTH is held
where a decision depends on it: spg-gll-ring-7 (m = 64) and spg-gll-chain-16-m10 (m = 10, 12 iterations) are non-monotone runs that lambda >= 20
keeps from converging, and each asserts that, once the ring is full, at least one decision would fall the other way with a ring one value
shorter and one with a ring one value longer (the replay counts them: Report.ring_short, ring_long); the call plans assert a step that only an
older value of the ring lets through at their boundary.  The other m = 10 cases run 6 iterations and see the ring only while it fills.  c1 = 0.6 where a second interpolation has to
land between sigma2 t and sigma2; `memoize` 0 and 1; tol 1e-10, so some runs end at a loop top (the stop rule is then checked too).

THE RECORD (not a tolerance; the assertion is ratio <= 1).  One run on one MI355X, tests/test_gpu_vec_replay.py::test_tally; nobody had
measured these ratios before.  Directions, gnorm, f, trial points, x_{k+1}, the sequence of evaluations, the counts and the stop rule: exact
in every case at every size.  No skipped iteration, no undecidable decision.  Worst |error| / bound per quantity (and the size it fell at):
    z (n > 5, norm-wise)   1.0e-02 (6)       4.0e-03 (7)       6.4e-04 (17)          1.3e-05 (130)
    decision, bound/margin 3.0e-12 (2048)    2.9e-13 (2^21+3)  7.3e-14 (2^19+2051)
    t                      1.7e-01 (5)       1.2e-01 (7)       1.7e-03 (2048)
    lambda                 1.5e-01 (2)       8.4e-04 (2048)    2.5e-06 (2^19+2051)   3.9e-07 (2^21+3)
    s_norm                 5.7e-01 (7)       2.3e-03 (2047)    4.6e-06 (2^19+2051)   3.7e-06 (2^21+3)
    y_norm                 3.3e-01 (6)       1.3e-01 (16)      2.3e-02 (130)
(the small sizes sit near 1 / (n + 2): one rounding against a bound of n + 2 of them.)  What the replay found on the library as it stood:
inside a callback ProjectedNewton's s_norm() / y_norm() still answered with the values of the previous minimize call (None in the first);
the pump now publishes them before the callback.  No kernel was wrong.
"""
import numpy as np

import spg_cases as S

INF = float("inf")
SMALL = (1, 2, 5, 6, 7, 15, 16, 17, 2047, 2048, 2049, 4099)
LARGE = ((1 << 19) + 2051, (1 << 21) + 3)
NEWTON_SIZES = (1, 2, 5, 6, 7, 15, 16, 17, 130)
DENSE_MAX = 130


def _rng(*k):
    return np.random.default_rng([int(v) for v in k])


def spd(n, scale=1.0, quartic=0.0):
    """-> fn(x) -> (f, g, H or None), x0"""
    rng = _rng(7, n)
    v = rng.standard_normal(n)
    v /= np.linalg.norm(v)
    dg = scale * np.logspace(0.0, -2.0, n)[rng.permutation(n)] if n > 1 else np.full(1, scale)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    h = None
    if n <= DENSE_MAX:
        r = np.eye(n) - 2.0 * np.outer(v, v)
        h = (r * dg) @ r
        h = 0.5 * (h + h.T)

    def fn(x):
        if h is not None:
            hx = h @ x
        else:
            w = dg * (x - 2.0 * v * float(v @ x))
            hx = w - 2.0 * v * float(v @ w)
        f, g, hh = 0.5 * float(x @ hx) - float(b @ x), hx - b, h
        if quartic:
            x2 = x * x
            f, g = f + 0.25 * quartic * float(x2 @ x2), g + quartic * x2 * x
            hh = h + 3.0 * quartic * np.diag(x2) if h is not None else None
        return f, g, hh
    return fn, x0


def crafted(n):
    j = np.arange(n) % 8
    rng = _rng(11, n)
    x0 = np.round(rng.uniform(-0.4, 0.4, n) * 256) / 256
    c = np.round(rng.uniform(-0.9, 0.9, n) * 256) / 256
    q = np.round(rng.uniform(0.25, 1.0, n) * 64) / 64
    lb, ub = np.full(n, -0.5), np.full(n, 0.5)
    for m, (xv, cv, qv) in {0: (-0.5, -1.0, 4.0), 1: (-0.5, 0.25, 0.5), 2: (0.5, 1.0, 4.0), 3: (0.5, -0.25, 0.5),
                            4: (-0.375, -0.4921875, 20.0), 5: (0.375, 0.4921875, 20.0)}.items():
        x0[j == m], c[j == m], q[j == m] = xv, cv, qv
    half = (np.arange(n) // 8) % 2 == 0
    lb[(j == 6) & half], ub[(j == 6) & ~half] = -INF, INF
    lb[j == 7], ub[j == 7] = -INF, INF

    # the line search's box: the solver's, but +-0.4375 on the unbounded entries, which creep towards +-0.75 and cross it at the fourth step
    x0[j == 7], c[j == 7], q[j == 7] = 0.0, np.where(half, 0.75, -0.75)[j == 7], 0.25
    llb, lub = np.where(j == 7, -0.4375, lb), np.where(j == 7, 0.4375, ub)

    def fn(x):
        e = x - c
        return 0.5 * float(np.sum(q * e * e)), q * e, None
    fn.ls_box = (llb, lub)
    return fn, x0, lb, ub


def huber(n):
    """pseudo-Huber with a tiny delta: |g| is about 1 everywhere, so a large lambda overshoots and the interpolated steps are rejected down to t <= 0.1"""
    rng = _rng(19, n)
    x0, dl = rng.uniform(0.1, 0.5, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0), 1e-3

    def fn(x):
        r = np.sqrt(1.0 + (x / dl) ** 2)
        return dl * float(np.sum(r - 1.0)), (x / dl) / r, None
    return fn, x0


def crossing(n):
    """a separable quadratic whose first projected-gradient step crosses the line search's upper bound 0.5 in every entry: the projected trial's
    ||xt - x||^2 is less than half the unprojected one's, and with c1 = 0.6 the decision at t = 1 depends on which of the two is used"""
    rng = _rng(23, n)
    q, c = rng.uniform(0.5, 1.0, n), rng.uniform(0.8, 1.2, n)

    def fn(x):
        e = x - c
        return 0.5 * float(np.sum(q * e * e)), q * e, None
    fn.ls_box = (np.full(n, -INF), np.full(n, 0.5))
    return fn, np.zeros(n)


def sep(n):
    """one numpy pass: f = sum a (x - c)^2 / 2 + (x - c)^4 / 4"""
    rng = _rng(13, n)
    a, c, x0 = rng.uniform(0.5, 2.0, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.5, 0.5, n)

    def fn(x):
        e = x - c
        e2 = e * e
        return float(np.sum(e2 * (0.5 * a + 0.25 * e2))), e * (a + e2), None
    return fn, x0


def chain(n):
    rng = _rng(5, n)
    a, x0 = rng.uniform(0.5, 2.0, n), rng.uniform(-2.0, 2.0, n)
    base = S.chain_fn(a, 0.3)
    return (lambda x: base(x) + (None,)), x0


def problem(case):
    """-> fn(x) -> (f, g, H), x0, lb, ub"""
    n, box = case["n"], case.get("box", INF)
    if case["prob"] == "crafted":
        return crafted(n)
    if case["prob"] == "tri":
        import sparse_cases as SC
        rng = _rng(17, n)
        indptr, cols, vals = SC.tri(n)
        b, x0 = rng.standard_normal(n), rng.standard_normal(n)

        def fn(x):  # (a host statement of the same function, for the CPU licence: the GPU run uses the device objective)
            hx = 2.04 * x
            hx[1:] -= x[:-1]
            hx[:-1] -= x[1:]
            return 0.5 * float(x @ hx) - float(b @ x), hx - b, None
        fn.csr, fn.b = (indptr, cols, vals), b
        return fn, x0, np.full(n, -box), np.full(n, box)
    if case["prob"] == "chain":
        fn, x0 = chain(n)
    elif case["prob"] == "huber":
        fn, x0 = huber(n)
    elif case["prob"] == "crossing":
        fn, x0 = crossing(n)
    elif case["prob"] == "sep":
        fn, x0 = sep(n)
    elif case["prob"] == "walled":  # inf beyond a radius: BackTracking multiplies t by beta without counting
        base, x0 = spd(n, scale=30.0)
        rad = 1.25 * float(np.max(np.abs(x0)))

        def fn(x):
            f, g, h = base(x)
            return (INF if float(np.max(np.abs(x))) > rad else f), g, h
    else:
        fn, x0 = spd(n, scale=case.get("scale", 1.0), quartic=1.0 if case["prob"] == "quartic" else 0.0)
    return fn, case.get("x0_scale", 1.0) * x0, np.full(n, -box), np.full(n, box)


def line_search(case, lb, ub, fn=None):
    """the search's settings as tests/vec_replay.py reads them"""
    kind = case["ls"]
    ls = dict(kind=kind, c1=case.get("c1", 1e-4), m=case.get("m", 3), sigma1=0.1, sigma2=0.9, beta=0.5, lo=None, hi=None)
    if "sigmas" in case:
        ls["sigma1"], ls["sigma2"] = case["sigmas"]
    if kind == "btb":  # a box of its own, narrower than the solver's on every second entry
        narrow = np.arange(lb.size) % 2 == 0
        w = case.get("ls_box", 0.25)
        ls["lo"], ls["hi"] = np.where(narrow, np.maximum(lb, -w), lb), np.where(narrow, np.minimum(ub, w), ub)
        if hasattr(fn, "ls_box"):
            ls["lo"], ls["hi"] = fn.ls_box
    return ls


def _case(name, method, ls, prob, n, **kw):
    c = dict(name=name, method=method, ls=ls, prob=prob, n=n, plan=(6,), memoize=0, tol=1e-10, max_ls=50, expect={})
    c.update(kw)
    return c


def _cases():
    out = []
    for i, n in enumerate(SMALL):
        out.append(_case(f"spg-gll-spd-{n}", "spg", "gll", "spd", n, box=(0.05 if i % 2 else INF), memoize=(i // 2) % 2, m=(1, 3, 10)[i % 3]))
        if n >= 16:
            out.append(_case(f"pgd-btb-crafted-{n}", "pgd", "btb", "crafted", n, memoize=(i + 1) % 2,
                             expect=dict(edges=True, moved=True, not_moved=True)))
            out.append(_case(f"spg-gll-crafted-{n}", "spg", "gll", "crafted", n, memoize=i % 2, expect=dict(edges=True)))
        else:
            out.append(_case(f"pgd-btb-spd-{n}", "pgd", "btb", "spd", n, box=0.5, ls_box=0.5, memoize=(i + 1) % 2))  # (the search holds the solver's box)
    # the non-convex chain: s.y < 0 clearing its bound; every branch of GLLQuadratic over these cases together
    out.append(_case("spg-gll-chain-2049", "spg", "gll", "chain", 2049, box=1.5, m=10, plan=(12,), x0_scale=0.2, expect=dict(neg_sy=True, interp=True)))
    out.append(_case("spg-gll-chain-17-m1", "spg", "gll", "chain", 17, box=1.5, m=1, plan=(12,), memoize=1))
    out.append(_case("spg-gll-spd4-4099-lambdas", "spg", "gll", "spd", 4099, scale=3.0, m=3, plan=(12,), lambdas=(0.5, 2.0),
                     expect=dict(clamp_lo=True, clamp_hi=True)))
    out.append(_case("spg-gll-chain-2047-steep", "spg", "gll", "chain", 2047, m=3, plan=(8,), lambdas=(50.0, 100.0), sigmas=(0.01, 0.9),
                     expect=dict(half_interp=True)))
    out.append(_case("spg-gll-huber-2047", "spg", "gll", "huber", 2047, m=1, plan=(6,), lambdas=(50.0, 100.0), expect=dict(halve=True)))
    out.append(_case("spg-gll-chain-16-narrow", "spg", "gll", "chain", 16, box=1.5, m=3, plan=(8,), lambdas=(5.0, 20.0), sigmas=(0.1, 0.5),
                     expect=dict(interp=True)))
    # a strict c1: a trial that gains less than 0.6 of the linear prediction is rejected, so a second interpolation lands between sigma2 t and sigma2
    out.append(_case("spg-gll-chain-17-strict", "spg", "gll", "chain", 17, box=1.5, m=1, c1=0.6, lambdas=(3.0, 10.0), expect=dict(interp=True, half_interp=True)))
    out.append(_case("spg-gll-chain-2048-strict", "spg", "gll", "chain", 2048, box=1.5, m=1, c1=0.6, lambdas=(3.0, 10.0), memoize=1,
                     expect=dict(interp=True, half_interp=True)))
    # BackTrackingB: every entry's first step crosses the search's bound, and c1 = 0.6 makes the decision at t = 1 depend on diff2
    for n in (17, 2049):
        out.append(_case(f"pgd-btb-crossing-{n}", "pgd", "btb", "crossing", n, c1=0.6, plan=(2,), memoize=1, expect=dict(moved=True)))
    # the ring of QN_GLL_MAX_M values fills and shifts: lambda >= 20 keeps SPG from converging on the chain in a narrow box, f goes up and down for
    # 70 iterations, and once the ring is full some decisions would fall the other way with a ring of 63 and of 65 values (counted by the replay)
    out.append(_case("spg-gll-ring-7", "spg", "gll", "chain", 7, box=0.75, x0_scale=0.2, m=64, plan=(70,), lambdas=(20.0, 100.0), tol=0.0,
                     expect=dict(ring_shifts=6, ring_short=True, ring_long=True)))
    # ... and the same for m = 10 inside 12 iterations: a ring of 9 and one of 11 values each change a decision of the last two iterations
    out.append(_case("spg-gll-chain-16-m10", "spg", "gll", "chain", 16, box=0.5, m=10, plan=(12,), lambdas=(20.0, 100.0), tol=0.0, memoize=1,
                     expect=dict(ring_short=True, ring_long=True)))
    # the ring across calls: a non-monotone run in three call plans, one x-trace
    for plan in ((6,), (3, 3), (1, 2, 3)):
        out.append(_case("spg-gll-plan-" + "-".join(map(str, plan)), "spg", "gll", "chain", 2049, box=1.5, m=3, plan=plan, memoize=1, x0_scale=0.2, group="plan",
                         expect=dict(nonmonotone_at=3)))
    # BackTracking, with a closure that is inf beyond a radius
    out.append(_case("pgd-bt-walled-17", "pgd", "bt", "walled", 17, expect=dict(nonfinite=True)))
    out.append(_case("spg-bt-walled-2049", "spg", "bt", "walled", 2049, memoize=1, lambdas=(5.0, 10.0), expect=dict(nonfinite=True)))
    out.append(_case("spg-bt-spd-4099", "spg", "bt", "spd", 4099, box=0.05))
    # the Newton pair
    for i, n in enumerate(NEWTON_SIZES):
        out.append(_case(f"pn-gll-quartic-{n}", "pn", "gll", "quartic", n, box=(0.3 if i % 2 and n != 6 else INF), plan=(4,), memoize=(i // 2) % 2))
        out.append(_case(f"spn-gll-quartic-{n}", "spn", "gll", "quartic", n, box=(0.3 if n in (2, 5, 16, 130) else INF), plan=(4,), memoize=(i + 1) % 2))
    out.append(_case("pn-bt-quartic-5", "pn", "bt", "quartic", 5, box=0.3, plan=(2, 2), memoize=1))
    out.append(_case("pn-btb-quartic-7", "pn", "btb", "quartic", 7, box=0.5, ls_box=0.5, plan=(4,)))
    out.append(_case("spn-btb-quartic-16", "spn", "btb", "quartic", 16, box=0.5, ls_box=0.5, plan=(4,), memoize=1))
    # the large sizes: three iterations on closures of one numpy pass
    for n in LARGE:
        out.append(_case(f"spg-gll-sep-{n}", "spg", "gll", "sep", n, box=0.4, plan=(3,), memoize=1))
        out.append(_case(f"pgd-btb-sep-{n}", "pgd", "btb", "sep", n, box=0.4, ls_box=0.35, plan=(3,), memoize=1))
        out.append(_case(f"spg-tri-{n}", "spg", "gll", "tri", n, box=0.5, plan=(3,), memoize=1, limited=True))
    return out


CASES = _cases()
BRANCHES = ("accept", "halve", "interp", "half_interp")


def check_conditions(case, rep):
    """what the case was chosen for, asserted on the replay's own counts"""
    e = case["expect"]
    for b in BRANCHES:
        if e.get(b):
            assert rep.branches[b] >= 1, (case["name"], b, rep.branches)
    for q in ("neg_sy", "clamp_lo", "clamp_hi", "moved", "not_moved", "ring_short", "ring_long"):
        if e.get(q):
            assert getattr(rep, q) >= 1, (case["name"], q)
    if e.get("nonfinite"):
        assert rep.branches["nonfinite"] >= 1, (case["name"], rep.branches)
    if "nonmonotone_at" in e:  # f rises over this iteration: the step is accepted against an older value of the ring (the call boundary of the plans)
        assert e["nonmonotone_at"] in rep.nonmonotone_at, (case["name"], rep.nonmonotone_at)
    if e.get("ring_shifts"):
        assert rep.ring_shifts >= e["ring_shifts"], (case["name"], rep.ring_shifts)
    if e.get("edges"):  # at x0 and again after the first step: entries on lb pushed outward and inward, the same on ub
        assert all(v > 0 for v in rep.edges[0]) and all(v > 0 for v in rep.edges[1]), (case["name"], rep.edges[:2])
    assert rep.iterations >= 1
