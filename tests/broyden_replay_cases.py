"""Broyden / BroydenB runs on device quadratics, replayed in extended precision entry by entry: what tests/test_ref_broyden_replay.py (CPU: licenses
the checker on a float64 restatement in three summation orders and on seven planted faults) and tests/test_gpu_broyden_replay.py (GPU) share.  Test
infrastructure: the product does not import this file.  The replay is tests/qn_replay.py (method "broyden": its docstring derives the update's
bound and the lazy direction's); truth, bounds, problems, box and segment plans are tests/quad_replay_cases.py's.

WHY.  r1_pass_kernel (csrc/qn_rank1.hip.h) is the one kernel here that holds a non-symmetric H and sums columns (w = H' s); it applies the pending
update, writes the tile back and forms two row sums from the same registers, in seven instantiations (qn_host_rank1.hip.h: keys 2, 4, 5, 6, 7, 9,
11).  tests/test_gpu_broyden.py holds whole windows to a tolerance relative to the compared array's largest magnitude, which cannot see a wrong
entry that is small beside max |H|.  Here every entry of every step and of every stored matrix has its own bound.

THE SIZES, each the smallest at which its mechanism exists (QN_R1_TB = 128, n_pad a multiple of 16):
    7     n_pad = 16: one ragged tile                         128   one exactly full tile, nb = 1
    129   n_pad = 144: the edge tile has ONE live column, 15 padded ones, and lanes 8 .. 63 outside the matrix
    257   n_pad = 272: nb = 3, a ragged third tile, r1_reduce_kernel folds three partials
    384   nb = 3, full tiles                                  1024  nb = 8 (one segment of three, both memoize settings, `synth` only)

WHICH INSTANCE RUNS WHERE (r1_enqueue_req; a call never continues warm on this path, so it opens with an evaluation and a direction pass).
memoize = 0: every iteration is a direction pass (key 4, with an update pending 6) and an update pass with one right-hand side (5; 7 is the update
pass with ONE right-hand side that finds an update pending: with memoize = 0 the direction pass in front of it has always applied the update,
QN_ST_AFTER_DIR clears `pending`, so no minimize call reaches 7 and it is not replayed here; the README says so).  memoize = 1: one direction pass per call
(4, or 6 when the call before left an update pending: the warm plans), then one update pass per iteration with two right-hand sides (9 the first of
a run, 11 with the previous update pending) and the lazy direction d+ = -(v + c a (w . g+)) of the control step.  The getter between the calls of a
plan flushes the pending update (2).  Passes per call of K updating iterations: K + 1 (memoize = 1) or 2 K (memoize = 0), of which K - 1 found an
update pending, one more when the call was entered with one.

THE RESTATEMENT.  BroydenRef: RefSolver's loop (box, Armijo backtracking) with H + c (s - H y)(H' s)', c = 1 / s.y, in the three orders; the
blocked order mimics the kernel: 128 x 128 tiles of the FULL matrix, row partials folded over the tile columns in ascending order, column partials
over the tile rows.  lazy = True forms every direction but a call's first as the control step does with memoize = 1.  PLANTED FAULTS:
      ("w_rows",)              w = H s instead of H' s (invisible on the first update from I: segments restart from a matrix read back)
      ("textbook_den",)        the denominator is s'Hy
      ("col_row_dropped", i)   row i missing from the column sums of the update of iteration 1
      ("edge_entry", k)        entry (n - 1, n - 1) of H left as it was by the update of iteration k
      ("applied_twice", k)     the pending update of iteration k (a call's last) applied by the getter's flush and again by the next call's first pass
      ("stale_dir", k)         the direction of iteration k formed without the latest update
      ("lazy_sg",)             the lazy direction with s.g+ where w.g+ belongs
      ("g_entry", k, rel)      as tests/quad_replay_cases.py

THE CASES (GPU_CASES below; the CPU file runs the restatement on every distinct (problem, n, box, lazy, plan) of them):
    Broyden + More-Thuente / backtracking, `synth`, every size, memoize 0 and 1, every plan of PLANS and WARM_PLANS (n = 1024: one segment of three)
    Broyden + More-Thuente, `nonsym` and `wide`, n = 129, 257, memoize 1, plans (3, 3) and (1, 2, 3)
    BroydenB + MoreThuenteB / BackTrackingB in the box, `synth` and `wide`, n = 129, 257, memoize 0 and 1, plan (3, 3)
Nothing is dropped or shortened.  (`wide`, n = 7, BroydenB + BackTrackingB stops after three iterations, the third without an update; the box runs at
n = 129 and 257 only, so that combination is not among the cases.)

THE RECORD: worst asserted ratio per (size, check).  CPU: the float64 restatement, three orders, lazy and not, every case above.  GPU: one run of
tests/test_gpu_broyden_replay.py on one MI355X, printed by its last test.  A record of one run each, not a tolerance.
         n      f        gnorm    s_norm   y_norm   dir      H
    CPU  7      2.9e-2   4.5e-2   9.3e-2   4.1e-2   7.3e-2   3.0e-2
    GPU  7      4.7e-2   4.1e-2   9.3e-2   3.3e-2   5.9e-2   2.0e-2
    CPU  128    2.1e-2   7.4e-3   6.7e-3   5.8e-3   2.3e-2   3.7e-2
    GPU  128    4.3e-3   3.7e-3   6.4e-3   3.1e-3   3.4e-2   3.7e-2
    CPU  129    2.6e-2   1.5e-2   7.4e-3   7.9e-3   1.2e-1   3.7e-2
    GPU  129    6.8e-3   4.6e-3   8.3e-3   6.9e-3   1.2e-1   4.1e-2
    CPU  257    1.2e-2   9.5e-3   3.8e-3   6.3e-3   1.2e-1   4.0e-2
    GPU  257    3.4e-3   3.7e-3   3.8e-3   3.3e-3   1.2e-1   3.9e-2
    CPU  384    6.2e-3   2.5e-3   2.4e-3   2.0e-3   2.1e-2   3.0e-2
    GPU  384    1.1e-3   1.2e-3   2.4e-3   1.0e-3   2.1e-2   3.2e-2
    CPU  1024   1.8e-3   6.5e-4   0        3.8e-4   9.9e-3   2.9e-2
    GPU  1024   3.4e-4   3.5e-4   5.7e-4   3.5e-4   1.1e-2   3.4e-2
(0.12: a step of the twelve-decade problem `wide`.)  CPU: 0 of 6444 triples skipped.  GPU: 4 of 4036, the direction of iteration 1 of the first
segment of the four `wide` BroydenB + MoreThuenteB runs, whose half-width exceeds CAP of the step; nothing failed on the library as it stood.
The single-update test of tests/test_gpu_broyden.py on the same run: 2.2e-2 of its bound at the most (n = 7, the matrix over twelve decades)."""
import numpy as np

import quad_replay_cases as Q
from quad_replay_cases import TB

SIZES = [7, 128, 129, 257, 384, 1024]
NPAD = {7: 16, 128: 128, 129: 144, 257: 272, 384: 384, 1024: 1024}
FAULT_SIZES = [7, 129, 257]
NOT_SYMMETRIC = 1e6   # max |H - H'| must exceed this many times max DH: the matrix read back is clearly not symmetric


def plans(n):
    """[(plan, read_h)]"""
    if n == 1024:
        return [((3,), True)]
    return [(p, True) for p in Q.PLANS] + [(p, False) for p in Q.WARM_PLANS]


def plan_id(v):
    return "+".join(map(str, v[0])) + ("" if v[1] else "warm")


# (kind, n, line search, boxed, memoize, (plan, read_h))
GPU_CASES = [("synth", n, ls, False, m, pl) for n in SIZES for ls in ("mt", "bt") for m in (0, 1) for pl in plans(n)]
GPU_CASES += [(kind, n, "mt", False, 1, (p, True)) for kind in ("nonsym", "wide") for n in (129, 257) for p in ((3, 3), (1, 2, 3))]
GPU_CASES += [(kind, n, ls, True, m, ((3, 3), True)) for kind in ("synth", "wide") for n in (129, 257) for ls in ("mtb", "btb") for m in (0, 1)]
# what the restatement (one line search: Armijo backtracking) has to carry: (kind, n, boxed, lazy, (plan, read_h))
REF_CASES = sorted({(k, n, bx, bool(m), pl) for k, n, _, bx, m, pl in GPU_CASES}, key=str)


# ---- the three orders of H v and H' v on a full, non-symmetric matrix ----
def _fold(parts):
    t = parts[0]
    for p in parts[1:]:
        t = t + p
    return t


def mvf(order, m, v):
    """m @ v.  "blocked": per 128 x 128 tile the rows' partial sums, folded over the tile columns in ascending order (r1_reduce_kernel)"""
    if order == "plain":
        return m @ v
    if order == "reversed":
        return Q._rsum(m * v)
    n = v.size
    return _fold([m[:, j:j + TB] @ v[j:j + TB] for j in range(0, n, TB)])


def mtv(order, m, v, skip_row=None):
    """m' @ v, the column sums.  "blocked": per tile the columns' partial sums, folded over the tile rows.  skip_row: that row left out (a fault)"""
    if skip_row is not None:
        v = v.copy()
        v[skip_row] = 0.0
    if order == "plain":
        return v @ m
    if order == "reversed":
        return Q._rsum((m * v[:, None]).T)
    n = v.size
    return _fold([v[i:i + TB] @ m[i:i + TB] for i in range(0, n, TB)])


class BroydenRef(Q.RefSolver):
    """A float64 Broyden / BroydenB run in the library's layout (RefSolver's records, box and backtracking), the module docstring's faults"""

    def __init__(self, q, b, x0, order="plain", box=None, fault=None, lazy=False):
        super().__init__(q, b, x0, "broyden", order, box=box, fault=fault)
        self.lazy, self.hg_lazy, self.twice = lazy, None, None

    def _gdir(self, g, k):
        ft = self.fault
        gd = g.copy()
        if ft[0] == "g_entry" and ft[1] == k:
            j = int(np.argmax(np.abs(gd)))
            gd[j] += ft[2] * abs(gd[j])
        return gd

    def advance(self, iters):
        ft, o = self.fault, self.order
        self.hg_lazy = None           # a call opens with a pass over H
        if self.twice is not None:    # (the getter returned the right matrix; the pass applies the update again)
            self.h, self.twice = self.twice, None
        for _ in range(iters):
            x, f, g, k = self.x, self.f, self.g, self.k
            if self.hg_lazy is not None:
                hg = self.hg_lazy
            else:
                hg = mvf(o, self.h_before if (ft[0] == "stale_dir" and ft[1] == k) else self.h, self._gdir(g, k))
            if self.box is None:
                d = -hg
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
            h = self.h
            u = mvf(o, h, y)
            if ft[0] == "w_rows":
                w = mvf(o, h, s)
            else:
                w = mtv(o, h, s, skip_row=ft[1] if (ft[0] == "col_row_dropped" and k == 1) else None)
            with np.errstate(all="ignore"):  # (a planted fault may stall the run: s.y = 0 gives a matrix that is not finite, which the replay rejects)
                c = np.float64(1.0) / np.float64(Q.dot(o, s, u) if ft[0] == "textbook_den" else Q.dot(o, s, y))
                a = s - u
                hn = h + c * np.outer(a, w)
            if ft[0] == "edge_entry" and ft[1] == k:
                hn[-1, -1] = h[-1, -1]
            if ft[0] == "applied_twice" and ft[1] == k:
                self.twice = hn + c * np.outer(a, w)
            if self.lazy:  # d+ = -(v + c a (w . g+)), v = H g+ by the update pass's second right-hand side
                gd = self._gdir(gn, k + 1)
                v = mvf(o, h, gd)
                self.hg_lazy = v if (ft[0] == "stale_dir" and ft[1] == k + 1) else v + c * (a * Q.dot(o, s if ft[0] == "lazy_sg" else w, gd))
            self.h_before, self.h = h, hn
            self.x, self.f, self.g, self.k = xn, fn, gn, k + 1


def ref_run(kind, n, boxed, lazy, plan, read_h, order, fault=None):
    """-> (reports, segments) of the restatement on one case"""
    q, b, x0 = Q.problem(kind, n)
    bx = Q.box(x0) if boxed else None
    rs = BroydenRef(q, b, x0, order, box=bx, fault=fault, lazy=lazy)
    segs = Q.run_plan(rs, rs.start(), plan, read_h)
    tag = f"{kind}{n}/broyden{'/box' if boxed else ''}/{'lazy' if lazy else 'pass'}/{plan_id((plan, read_h))}/{order}"
    return Q.replay_plan(tag, Q.truth_factory(kind, n), "broyden", segs, box=bx), segs


def asymmetry(h):
    h = np.asarray(h)
    return float(np.max(np.abs(h - h.T)))
