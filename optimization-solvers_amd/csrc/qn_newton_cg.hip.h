// qn_newton_cg.hip.h -- truncated Newton (QN_NEWTON_CG) on the first-order family's machine (qn_vec.hip.h): phase QN_VP_NSOLVE with Newton's
// direction from a few conjugate-gradient steps on H z = g, where L-BFGS has z = H_k g.  Each inner step costs ONE product q = H p of the
// log-sum-exp objective -- one stream of A, never a matrix (qn_lse_hv.hip.h).  Unbounded only; the only objective is log-sum-exp.
//
// THE RULES, in this order (tests/ref_newton_cg.py restates them operation for operation):
//   1. p = softmax(A x_k + c) and gbar = A'p by lse_enqueue_weights (two passes of A: the loop top's one-pass evaluation keeps no normalised p);
//   2. tn_init_kernel: z = 0, r = g, p = g, the shares of gg = g.g (and a copy of gbar: an evaluation overwrites the objective's);
//      tn_start_kernel: rr = gg, j = 0, eta = min(eta_max, sqrt(sqrt(gg))) (IEEE sqrt; min is a comparison);
//   3. q = H p (lse_hv_onepass_kernel, lse_hv_combine_kernel), kappa = p.q;
//   4. tn_step_kernel: unless kappa > 0 and finite: neg_curv += 1, z = g if j == 0, the loop ends;
//   5. alpha = rr / kappa; tn_update_kernel: z += alpha p, r -= alpha q (alpha p and alpha q round first, no FMA), the shares of rr' = r.r and of
//      g.z; tn_commit_kernel: j += 1;
//   6. sqrt(rr') <= eta sqrt(gg) (the product rounds): the loop ends (tolerance); else j == max_inner: it ends (cap);
//   7. beta = rr' / rr; tn_next_kernel: p = r + beta p (beta p rounds first); rr = rr'; back to 3;
//   8. behind the loop: g.z > 0 and finite, or else z = g and fallbacks += 1 (L-BFGS's safeguard; after rule 4 at j = 0 z IS g and the test is
//      not made); tn_dir_kernel writes d = -z directly, as cg_dir_kernel does -- never through P(x - z) - x -- and in the same launch the shares
//      ||g||_inf, g.d, ||d||_inf where vec_dir_kernel leaves them; tn_top_kernel is the second half of the loop top (vec_top_kernel's: g.d,
//      t = 1, StrongWolfe's start, phase QN_VP_TRIAL).
// Inner products: product and sum round separately, G = vec_grid(n_pad) shares added in index order (vec_sum_parts) -- the family's convention.
//
// WHO WRITES THE CONTROL BLOCK.  Only one-workgroup kernels do (start, step, commit, top); the device-wide ones (init, update, next, dir) read
// it.  That is why rules 5-7 are three launches and not two: a device-wide kernel whose first workgroup committed rr while the others still
// read it would race.  Per inner step: the two product launches, step, update, commit, next.
//
// PREDICATION.  Every launch returns at once unless the phase is QN_VP_NSOLVE, the method is this one and tn_state says what it needs: init
// and start run in the batch that saw the loop top pass (they are enqueued in no other); the inner step's launches need QN_TN_RUNNING; dir and
// top need QN_TN_ENDED.  A loop that is still running when a batch's inner steps are used up leaves the phase at QN_VP_NSOLVE: dir, top and the
// rest of the iteration return, the host peeks, and the next batch starts with another chunk of inner steps (qn_host_newton_cg.hip.h).
// Profiling mode, this method: t_newton_ms = the product launches, t_hpass_ms = the device-wide tn_* streams, t_ereduce_ms = the weights at x_k
// (four launches, two passes of A), the rest under t_ctl_ms.
//
// THE JACOBI PRECONDITIONER (qn_solver_set_newton_cg_preconditioner, QN_PRECOND_JACOBI; tests/ref_newton_pcg.py restates it).  QN_PRECOND_NONE runs
// the launches above and nothing else.  With Jacobi these rules change:
//   1'. behind the weights at x_k, the kind's diagonal pass (its table's `hess_diag`: M_j = H(x_k)_jj and minv into the solver's two vectors),
//       once per outer iteration, unpredicated like the weights (it writes the objective's scratch and those two vectors only);
//   2'. minv_j = 1 / M_j by IEEE division when M_j > 0 and finite, else minv_j = 1 (written by the diagonal's own launch: hd_minv); entries
//       n .. n_pad hold a finite value, and z, r, p stay exactly 0 there because g is.  tn_pinit_kernel: z = 0, r = g, p = minv o g (one rounding),
//       the shares of gg = g.g, of rz = sum r_j (minv_j r_j) (the inner product rounds first) and of the count of substituted entries;
//       tn_start_kernel: rz beside rr = gg, floored_last; eta is unchanged;
//   5'. alpha = rz / kappa; tn_pupdate_kernel: z += alpha p, r -= alpha q, and in the same pass the shares of rr' = r.r, rz' = r.(minv o r), g.z;
//   6.  unchanged: sqrt(rr') <= eta sqrt(gg) on the EUCLIDEAN residual -- the forcing term means the same with and without the preconditioner;
//   7'. beta = rz' / rz; tn_pnext_kernel: p = minv o r + beta p (both products round first); rz = rz'.  y = minv o r is never stored: the update
//       and the next-direction streams each read minv, 8 n bytes more apiece.
// Rules 3, 4 and 8, the chunk, the predication and who writes the control block are unchanged.  The preconditioned streams are SIBLINGS of init,
// update and next: the plain kernels keep their operations and their order.  The one-workgroup kernels read tn_precond and keep rz beside rr.
// Profiling mode: the diagonal pass is timed with the weights, under t_ereduce_ms.
#pragma once

#define QN_TN_NPART 5 // tpart[q * QN_VEC_MAXG + b]: 0 g.g, 1 r.r, 2 g.z; Jacobi: 3 r.(minv o r), 4 the count of substituted entries of minv

struct QnTnArgs {
    double *r, *p, *q;     // the residual, the inner direction, H p: n_pad each
    double* gbar;          // the method's copy of A'p
    const double* gbar_src; // the objective's (its table's `gbar`: lse.gall as lse_enqueue_weights left it, or zeros)
    double* tpart;         // [QN_TN_NPART][QN_VEC_MAXG]
    const double* kshares; // lse_hv_combine_kernel's shares of p.q
    int kcount;
    const double *mdiag, *minv; // Jacobi: M = diag H(x_k) and rule 2''s 1 / M, n_pad each (NULL without a preconditioner)
};

__device__ __forceinline__ bool tn_mine(const QnVecCtl* c) { return c->phase == QN_VP_NSOLVE && c->method == QN_NEWTON_CG; }

// rule 2, the streams: z = 0, r = g, p = g, gbar copied, the shares of g.g
__global__ __launch_bounds__(QN_VEC_TPB) void tn_init_kernel(const QnVecArgs a, const QnTnArgs t) {
    __shared__ double lds[64];
    if (!tn_mine(a.ctl)) return;
    double gg[1] = {0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d g = ld2(a.g + 2 * j);
        st2(a.zw + 2 * j, (v2d){0.0, 0.0});
        st2(t.r + 2 * j, g);
        st2(t.p + 2 * j, g);
        st2(t.gbar + 2 * j, ld2(t.gbar_src + 2 * j));
        gg[0] = gg[0] + g.x * g.x;
        gg[0] = gg[0] + g.y * g.y;
    }
    ctl_block_sum<1>(gg, lds);
    if (threadIdx.x == 0) t.tpart[0 * QN_VEC_MAXG + blockIdx.x] = gg[0];
}

// rule 2, the scalars
__global__ __launch_bounds__(QN_VEC_TPB) void tn_start_kernel(const QnVecArgs a, const QnTnArgs t) {
    __shared__ double lds[64];
    QnVecCtl* c = a.ctl;
    if (!tn_mine(c)) return;
    const double gg = vec_sum_parts(t.tpart, 0, a.G, lds);
    const bool jacobi = c->tn_precond != 0; // (the same for every thread: the sums below are the whole workgroup's)
    double rz = 0.0, floored = 0.0;
    if (jacobi) {
        rz = vec_sum_parts(t.tpart, 3, a.G, lds);
        floored = vec_sum_parts(t.tpart, 4, a.G, lds); // (a sum of counts: exact)
    }
    if (threadIdx.x != 0) return;
    const double sq = sqrt(gg), s4 = sqrt(sq);
    c->tn_gg = gg; c->tn_sqgg = sq; c->tn_rr = gg;
    if (jacobi) { c->tn_rz = rz; c->tn_floored_last = (uint64_t)floored; c->tn_diag_passes++; }
    c->tn_eta = s4 < c->tn_eta_max ? s4 : c->tn_eta_max;
    c->tn_j = 0; c->tn_exit = 0; c->tn_zg = 0; c->tn_use_g = 0; c->tn_gz = 0.0;
    c->tn_state = QN_TN_RUNNING;
}

// the loop has ended (thread 0 of a one-workgroup kernel): rule 8's decision and the counters
__device__ __forceinline__ void tn_end(QnVecCtl* c, int why) {
    c->tn_exit = why;
    c->tn_inner_last = (uint64_t)c->tn_j; c->tn_inner_total += (uint64_t)c->tn_j;
    if (c->tn_zg) {
        c->tn_use_g = 1;
    } else {
        const double gz = c->tn_gz;
        c->tn_use_g = (gz > 0.0 && !isinf(gz)) ? 0 : 1;
        if (c->tn_use_g) c->tn_fallbacks++;
    }
    c->tn_state = QN_TN_ENDED;
}

// rules 3 (kappa from the product's shares), 4 and 5's scalar
__global__ __launch_bounds__(QN_VEC_TPB) void tn_step_kernel(const QnVecArgs a, const QnTnArgs t) {
    __shared__ double lds[64];
    QnVecCtl* c = a.ctl;
    if (!tn_mine(c) || c->tn_state != QN_TN_RUNNING) return;
    const double kappa = lse_hv_sum_shares(t.kshares, t.kcount, lds);
    if (threadIdx.x != 0) return;
    c->tn_kappa = kappa;
    c->tn_hv_passes++;
    if (!(kappa > 0.0) || isinf(kappa)) {
        c->tn_neg_curv++;
        if (c->tn_j == 0) c->tn_zg = 1;
        tn_end(c, QN_TN_EXIT_NEGCURV);
        return;
    }
    c->tn_alpha = (c->tn_precond ? c->tn_rz : c->tn_rr) / kappa; // rule 5 / 5'
}

// rule 5, the streams: 40 n bytes read (z, r, p, q, g), 16 n written (z, r)
__global__ __launch_bounds__(QN_VEC_TPB) void tn_update_kernel(const QnVecArgs a, const QnTnArgs t) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (!tn_mine(c) || c->tn_state != QN_TN_RUNNING) return;
    const double alpha = c->tn_alpha;
    double acc[2] = {0.0, 0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        v2d z = ld2(a.zw + 2 * j), r = ld2(t.r + 2 * j);
        const v2d p = ld2(t.p + 2 * j), q = ld2(t.q + 2 * j), g = ld2(a.g + 2 * j);
        const double ap0 = alpha * p.x, ap1 = alpha * p.y; // `alpha p` rounds first
        const double aq0 = alpha * q.x, aq1 = alpha * q.y;
        z.x = z.x + ap0; z.y = z.y + ap1;
        r.x = r.x - aq0; r.y = r.y - aq1;
        st2(a.zw + 2 * j, z);
        st2(t.r + 2 * j, r);
        acc[0] = acc[0] + r.x * r.x;
        acc[0] = acc[0] + r.y * r.y;
        acc[1] = acc[1] + g.x * z.x;
        acc[1] = acc[1] + g.y * z.y;
    }
    ctl_block_sum<2>(acc, lds);
    if (threadIdx.x == 0) {
        t.tpart[1 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        t.tpart[2 * QN_VEC_MAXG + blockIdx.x] = acc[1];
    }
}

// rules 5 (j += 1), 6 and 7's scalar
__global__ __launch_bounds__(QN_VEC_TPB) void tn_commit_kernel(const QnVecArgs a, const QnTnArgs t) {
    __shared__ double lds[64];
    QnVecCtl* c = a.ctl;
    if (!tn_mine(c) || c->tn_state != QN_TN_RUNNING) return;
    const double rrn = vec_sum_parts(t.tpart, 1, a.G, lds);
    const double gz = vec_sum_parts(t.tpart, 2, a.G, lds);
    const bool jacobi = c->tn_precond != 0;
    double rzn = 0.0;
    if (jacobi) rzn = vec_sum_parts(t.tpart, 3, a.G, lds);
    if (threadIdx.x != 0) return;
    c->tn_j++;
    c->tn_gz = gz;
    const double rr = c->tn_rr;
    c->tn_rr = rrn;
    const double rz = c->tn_rz;
    if (jacobi) c->tn_rz = rzn;
    const double bound = c->tn_eta * c->tn_sqgg;
    if (sqrt(rrn) <= bound) { tn_end(c, QN_TN_EXIT_TOL); return; }
    if (c->tn_j >= c->tn_cap) { tn_end(c, QN_TN_EXIT_CAP); return; }
    c->tn_beta = jacobi ? rzn / rz : rrn / rr; // rule 7 / 7'
}

// rule 7, the stream: 16 n read, 8 n written
__global__ __launch_bounds__(QN_VEC_TPB) void tn_next_kernel(const QnVecArgs a, const QnTnArgs t) {
    const QnVecCtl* c = a.ctl;
    if (!tn_mine(c) || c->tn_state != QN_TN_RUNNING) return;
    const double beta = c->tn_beta;
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d r = ld2(t.r + 2 * j);
        v2d p = ld2(t.p + 2 * j);
        const double b0 = beta * p.x, b1 = beta * p.y; // `beta p` rounds first
        p.x = r.x + b0;
        p.y = r.y + b1;
        st2(t.p + 2 * j, p);
    }
}

// ---- the Jacobi preconditioner's streams: siblings of init, update and next (the head of this file, rules 2', 5', 7') ----
// rule 2': z = 0, r = g, p = minv o g, gbar copied; the shares of g.g, of r.(minv o r) and of the count of entries j < n whose M_j is not positive
// and finite.  32 n bytes read (g, gbar, M, minv), 32 n written
__global__ __launch_bounds__(QN_VEC_TPB) void tn_pinit_kernel(const QnVecArgs a, const QnTnArgs t) {
    __shared__ double lds[64];
    if (!tn_mine(a.ctl)) return;
    double acc[3] = {0.0, 0.0, 0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d g = ld2(a.g + 2 * j), mi = ld2(t.minv + 2 * j), md = ld2(t.mdiag + 2 * j);
        const v2d y = {mi.x * g.x, mi.y * g.y}; // `minv o g`: one rounding
        st2(a.zw + 2 * j, (v2d){0.0, 0.0});
        st2(t.r + 2 * j, g);
        st2(t.p + 2 * j, y);
        st2(t.gbar + 2 * j, ld2(t.gbar_src + 2 * j));
        acc[0] = acc[0] + g.x * g.x;
        acc[0] = acc[0] + g.y * g.y;
        acc[1] = acc[1] + g.x * y.x;
        acc[1] = acc[1] + g.y * y.y;
        if (2 * j < a.n && !(md.x > 0.0 && !isinf(md.x))) acc[2] = acc[2] + 1.0;
        if (2 * j + 1 < a.n && !(md.y > 0.0 && !isinf(md.y))) acc[2] = acc[2] + 1.0;
    }
    ctl_block_sum<3>(acc, lds);
    if (threadIdx.x == 0) {
        t.tpart[0 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        t.tpart[3 * QN_VEC_MAXG + blockIdx.x] = acc[1];
        t.tpart[4 * QN_VEC_MAXG + blockIdx.x] = acc[2];
    }
}

// rule 5', the streams: tn_update_kernel's operations in its order, and the share of r.(minv o r) beside r.r and g.z.  48 n bytes read, 16 n written
__global__ __launch_bounds__(QN_VEC_TPB) void tn_pupdate_kernel(const QnVecArgs a, const QnTnArgs t) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (!tn_mine(c) || c->tn_state != QN_TN_RUNNING) return;
    const double alpha = c->tn_alpha;
    double acc[3] = {0.0, 0.0, 0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        v2d z = ld2(a.zw + 2 * j), r = ld2(t.r + 2 * j);
        const v2d p = ld2(t.p + 2 * j), q = ld2(t.q + 2 * j), g = ld2(a.g + 2 * j), mi = ld2(t.minv + 2 * j);
        const double ap0 = alpha * p.x, ap1 = alpha * p.y; // `alpha p` rounds first
        const double aq0 = alpha * q.x, aq1 = alpha * q.y;
        z.x = z.x + ap0; z.y = z.y + ap1;
        r.x = r.x - aq0; r.y = r.y - aq1;
        st2(a.zw + 2 * j, z);
        st2(t.r + 2 * j, r);
        const double y0 = mi.x * r.x, y1 = mi.y * r.y; // `minv o r` rounds first
        acc[0] = acc[0] + r.x * r.x;
        acc[0] = acc[0] + r.y * r.y;
        acc[1] = acc[1] + g.x * z.x;
        acc[1] = acc[1] + g.y * z.y;
        acc[2] = acc[2] + r.x * y0;
        acc[2] = acc[2] + r.y * y1;
    }
    ctl_block_sum<3>(acc, lds);
    if (threadIdx.x == 0) {
        t.tpart[1 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        t.tpart[2 * QN_VEC_MAXG + blockIdx.x] = acc[1];
        t.tpart[3 * QN_VEC_MAXG + blockIdx.x] = acc[2];
    }
}

// rule 7', the stream: p = minv o r + beta p.  24 n read, 8 n written
__global__ __launch_bounds__(QN_VEC_TPB) void tn_pnext_kernel(const QnVecArgs a, const QnTnArgs t) {
    const QnVecCtl* c = a.ctl;
    if (!tn_mine(c) || c->tn_state != QN_TN_RUNNING) return;
    const double beta = c->tn_beta;
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d r = ld2(t.r + 2 * j), mi = ld2(t.minv + 2 * j);
        v2d p = ld2(t.p + 2 * j);
        const double y0 = mi.x * r.x, y1 = mi.y * r.y; // `minv o r` and `beta p` round first
        const double b0 = beta * p.x, b1 = beta * p.y;
        p.x = y0 + b0;
        p.y = y1 + b1;
        st2(t.p + 2 * j, p);
    }
}

// rule 8: d = -z (or -g), and the loop top's three shares exactly where vec_dir_kernel leaves them
__global__ __launch_bounds__(QN_VEC_TPB) void tn_dir_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (!tn_mine(c) || c->tn_state != QN_TN_ENDED) return;
    const bool use_g = c->tn_use_g != 0; // a BRANCH: a z that rule 4 or the safeguard discarded is not read
    double gm = 0.0, dm = 0.0, gd[1] = {0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d g = ld2(a.g + 2 * j);
        v2d d;
        if (use_g) {
            d.x = -g.x;
            d.y = -g.y;
        } else {
            const v2d z = ld2(a.zw + 2 * j);
            d.x = -z.x;
            d.y = -z.y;
        }
        st2(a.d + 2 * j, d);
        gm = fmax(gm, fmax(fabs(g.x), fabs(g.y)));
        dm = fmax(dm, fmax(fabs(d.x), fabs(d.y)));
        gd[0] = gd[0] + g.x * d.x;
        gd[0] = gd[0] + g.y * d.y;
    }
    gm = vec_block_max(gm, lds);
    __syncthreads();
    dm = vec_block_max(dm, lds);
    __syncthreads();
    ctl_block_sum<1>(gd, lds);
    if (threadIdx.x == 0) {
        a.part[0 * QN_VEC_MAXG + blockIdx.x] = gm;
        a.part[1 * QN_VEC_MAXG + blockIdx.x] = gd[0];
        a.part[2 * QN_VEC_MAXG + blockIdx.x] = dm;
    }
}

// the second half of the loop top, as vec_top_kernel runs it in phase QN_VP_NSOLVE for the methods whose direction is ready when it is
// launched: g.d, the first trial t = 1, StrongWolfe's start (no box: the clip is +inf), phase QN_VP_TRIAL
__global__ __launch_bounds__(QN_VEC_TPB) void tn_top_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    QnVecCtl* c = a.ctl;
    if (!tn_mine(c) || c->tn_state != QN_TN_ENDED) return;
    const double gd = vec_sum_parts(a.part, 1, a.G, lds);
    if (threadIdx.x != 0) return;
    c->gd = gd;
    c->t = 1.0;
    c->ls_i = 0;
    if (c->ls_kind == QN_LS_STRONG_WOLFE && !wolfe_start(c, gd, INFINITY)) return;
    if (c->max_iter_ls <= 0) vec_ls_return(c, false);
    else c->phase = QN_VP_TRIAL;
}
