"""Replay of an OWLQN run, iteration by iteration, in extended precision from the run's own pairs: tests/lbfgs_replay.py's `Memory` and
`Direction`, unchanged, applied to the pseudo-gradient v in place of g (tests/test_ref_owlqn.py licenses it on the float64 restatement,
tests/test_gpu_owlqn_replay.py applies it to the GPU).  Test infrastructure: the product does not import this file.

A run on a host closure can be rebuilt from the outside: the solver receives g from the closure bit for bit, v_k follows from (x_k, g_k, l1) by
rule 1 with one rounding per entry (the same bits in numpy), s = x_next - x and y = g_next - g are one subtraction each.  So every iteration is
checked ON ITS OWN: z = H_k v_k in numpy.longdouble with lbfgs_replay's bound dz, then x_{k+1} is predicted through rules 3 and 5, entry by entry:

  alignment   l1_j == 0: d_j = -z_j.  Otherwise the sign of z_j is known when |z_j| > dz_j: d_j = -z_j when it is v_j's, the exact 0.0 when not.
              |z_j| <= dz_j (and v_j != 0): UNDECIDED, both outcomes are accepted.
  trial       d_j = 0.0 exactly: x_next_j = x_j exactly.  Otherwise u_j = x_j + fl(t d_j) lies in the interval x_j - t z_j +- (t dz_j + three
              roundings); l1_j == 0: x_next_j must lie in it.  Otherwise, with xi_j from (x_j, v_j): the interval contains 0: UNDECIDED, x_next_j is
              0.0 or lies in the interval; the interval lies strictly on xi_j's side: x_next_j must lie in it; on the other side: x_next_j == 0.0.

The ratio of an entry is |x_next_j - centre| / radius for an interval, 0 or inf for an exact outcome, the smallest over its accepted outcomes;
an iteration's ratio is the largest over its entries and must be <= 1.  An iteration whose largest radius exceeds lbfgs_replay.CAP max_i |s_k,i|
proves nothing and is skipped.  The scalar checks are lbfgs_replay's: gamma() within its bound, stored_pairs() equal to the replayed count,
updated[k] against s.y > DBL_EPSILON y.y wherever that clears its rounding bound, a reset only where v.z is not above its bound.
CONDITIONS on a case (check_conditions): at most a fifth of the iterations skipped, at most 1 % of all entries undecided.
"""
import numpy as np

import lbfgs_replay as LR
import ref_owlqn as RO
from lbfgs_replay import CAP, EPS, INF, LD, Recorder  # noqa: F401


class Run(LR.Run):
    def __init__(self, m, unit, l1, x0, rec):
        n = np.asarray(x0).size
        super().__init__(m, unit, np.full(n, -np.inf), np.full(n, np.inf), x0, rec)
        self.l1 = np.full(n, float(l1)) if np.ndim(l1) == 0 else np.asarray(l1, dtype=np.float64)


def _ratio(err, rad):
    with np.errstate(all="ignore"):
        return np.where(rad > 0, err / np.where(rad > 0, rad, 1), np.where(err == 0, 0.0, INF))


def compare_step(d, mem, x, v, l1, xn, t):
    """(worst ratio, largest radius, undecided entries) over the elements, chunk by chunk"""
    ratio = bound = 0.0
    undecided = 0
    tl, t64, k = LD(t), float(t), d.k
    coef = np.concatenate(([LD(d.gamma)], d.a, d.b)).astype(LD)
    cmag, cerr = np.abs(coef).astype(np.float64), np.concatenate(([d.c_g], d.c_y, d.c_s)).astype(np.float64)
    for c in LR._chunks(x.size):
        xc, vc, wc, xnc = x[c], v[c], l1[c], xn[c]
        xl = xc.astype(LD)
        if k == 0:
            z, za, dz = vc.astype(LD), np.abs(vc), np.zeros(xl.size)
        else:
            rows = [vc] + [y[c] for y in mem.Y] + [s[c] for s in mem.S]
            wide = np.empty((2 * k + 1, xl.size), dtype=LD)
            for i, r in enumerate(rows):
                wide[i, :] = r
            mags = np.abs(np.stack(rows))
            z, za, dz = np.dot(coef, wide), cmag @ mags * (1.0 + 1e-12), cerr @ mags
        smooth = wc == 0.0
        z64 = z.astype(np.float64)
        known = np.abs(z64) > dz * (1.0 + 1e-12)
        same = known & (((z64 > 0) & (vc > 0)) | ((z64 < 0) & (vc < 0)))
        und_align = ~smooth & ~known & (vc != 0.0)
        moves = smooth | same | und_align           # d = -z is an accepted outcome
        stays = (~smooth & ~same) | und_align       # d = 0.0 is
        # d = -z: fl(t d), then fl(x + .)
        pr = t64 * dz + EPS * t64 * (za + dz)
        rad = (pr + EPS * (np.abs(xc) + t64 * (za + dz) + pr)) * (1.0 + 1e-12)
        mid = xl - tl * z
        lo, hi = (mid - rad).astype(np.float64), (mid + rad).astype(np.float64)
        pos, neg = (xc > 0) | ((xc == 0) & (vc < 0)), (xc < 0) | ((xc == 0) & (vc > 0))
        contains0 = (lo <= 0) & (hi >= 0)
        inside = (pos & (lo > 0)) | (neg & (hi < 0))
        r_int = _ratio(np.abs(xnc - mid).astype(np.float64), rad)
        r_zero = np.where(xnc == 0.0, 0.0, INF)
        r_move = np.where(smooth, r_int, np.where(contains0, np.minimum(r_int, r_zero), np.where(inside, r_int, r_zero)))
        r_stay = np.where(xnc == xc, 0.0, INF)
        r = np.where(moves & stays, np.minimum(r_move, r_stay), np.where(moves, r_move, r_stay))
        undecided += int(np.count_nonzero(und_align | (moves & ~smooth & contains0)))
        ratio = max(ratio, float(np.max(r)))
        bound = max(bound, float(np.max(np.where(moves, rad, 0.0))))
    return ratio, bound, undecided


def replay(run):
    """lbfgs_replay.replay's loop with v in g's place and compare_step above; the report also counts `undecided` of `entries`"""
    assert run.t and all(t > 0.0 for t in run.t), "the replay needs at least one iteration and positive steps"
    rep, mem = LR.Report(), LR.Memory(run.m)
    rep.undecided = rep.entries = 0
    x, g = run.x0, run.rec.grad(run.x0, "x_0")
    resets = 0
    for k, (xn, t, upd, (stored, gam_dev, res_dev)) in enumerate(zip(run.xs, run.t, run.updated, run.states)):
        gnext = run.rec.grad(xn, f"x_{k + 1}")
        assert res_dev in (resets, resets + 1), (k, res_dev, resets)
        was_reset = res_dev > resets
        resets = res_dev
        v = RO.pseudo_gradient(x, g, run.l1)
        d = LR.Direction(mem, v, run.unit)
        rep.max_k = max(rep.max_k, len(mem))
        vz, dvz = float(d.gz), d.dgz
        if was_reset:
            if not len(mem):
                rep.problems.append((k, INF, "a reset with an empty memory"))
            elif np.isfinite(vz) and np.isfinite(dvz) and vz > dvz:
                rep.problems.append((k, vz / dvz if dvz > 0.0 else INF, f"reset although v.z = {vz:.3e} > its bound {dvz:.3e}"))
            mem.clear()
            d.plain()
            rep.resets += 1
        elif len(mem) and np.isfinite(dvz) and vz < -dvz:
            rep.problems.append((k, -vz / dvz if dvz > 0.0 else INF, f"no reset although v.z = {vz:.3e} < -{dvz:.3e}"))
        if np.isfinite(d.dgam) and abs(gam_dev - d.gamma) > d.dgam:
            rep.problems.append((k, abs(gam_dev - d.gamma) / d.dgam if d.dgam > 0.0 else INF, f"gamma {gam_dev!r} against {d.gamma!r} +- {d.dgam:.3e}"))
        s = xn - x
        smax = float(np.max(np.abs(s)))
        ratio, bound, und = compare_step(d, mem, x, v, run.l1, xn, t) if d.bounded else (INF, INF, 0)
        asserted = not bound > CAP * smax
        rep.worst_cap = max(rep.worst_cap, bound / smax if smax > 0.0 else (0.0 if bound == 0.0 else INF))
        rep.ratios.append(ratio)
        rep.asserted.append(asserted)
        rep.skipped += 0 if asserted else 1
        rep.undecided += und if asserted else 0
        rep.entries += x.size
        y = gnext - g  # rule 7: the SMOOTH gradients
        ex, mag = LR.cross([s, y], [y])
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
    print(rep.line(name) + f", undecided {rep.undecided} of {rep.entries} entries")
    assert not rep.problems, (name, rep.problems[:3])
    bad = [(k, r) for k, (r, a) in enumerate(zip(rep.ratios, rep.asserted)) if a and not r <= 1.0]
    assert not bad, (name, bad[:5])
    check_conditions(rep, name)


def check_conditions(rep, name):
    assert 5 * rep.skipped <= rep.iterations, (name, rep.skipped, rep.iterations)
    assert 100 * rep.undecided <= rep.entries, (name, rep.undecided, rep.entries)
