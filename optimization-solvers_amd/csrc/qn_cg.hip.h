// qn_cg.hip.h -- nonlinear conjugate gradient (QN_NONLINEAR_CG) on the first-order family's machine (qn_vec.hip.h): phase QN_VP_NSOLVE with the
// direction d+ = beta d - g+ where L-BFGS has z = H_k g.  Unbounded only: the direction is written as it is and never goes through
// d = P(x - z) - x, which would cost eps |x| per element and buys nothing without a box.
//
//   cg_dir_kernel      ONE stream: p <- beta p - g (beta p rounds first, then the difference; no FMA), or p <- -g when beta == 0 or no p exists (a
//                      BRANCH: a stale or unset p is never multiplied by zero); d <- p; the shares 0, 1, 2 of part[][] -- ||g||_inf, g.d, ||d||_inf --
//                      exactly where vec_dir_kernel leaves them, so vec_top_kernel's second half (gd, t = 1, wolfe_start) runs unchanged.
//                      16 n bytes read (g, p), 16 n written (p, d); 8 n read on the beta == 0 branch.
//   cg_accept_kernel   vec_accept_kernel for this method -- the same x_next, s, g <- gt, x <- x_next and x-trace arithmetic, operation for operation --
//                      which holds g, g+ and d in registers and so leaves, beside s.y and s.s, the shares of the eight sums every variant's beta is
//                      made of: g+.g+, g+.y, d.y, g+.d, y.y, d.d, g.g, g+.g.  The direction update has NO reduction launch of its own.
//                      32 n bytes read (x, d, g, gt), 16 n written (x, g): vec_accept_kernel's bytes.
//   [vec_post_kernel]  its branch for this method (cg_post, below): adds the shares in index order, rules 2-6 in thread 0, beta and the counters
//                      into QnVecCtl, `updated` = beta != 0.
//
// WHY p IS A BUFFER OF ITS OWN.  The loop top's vec_dir_kernel stores P(x - g) - x into d (it serves the projected gradient's norm) before
// cg_dir_kernel runs, so the direction just searched does not survive in d: it lives in cg_p, n_pad doubles, updated in place.  A cut that saves
// the second store (the machine reading its direction from cg_p) would need the trial, phi and accept kernels to learn a second direction pointer
// per method; it was not taken, so that no other method's launch changes.
//
// THE RULES, in this order (tests/ref_cg.py applies them in the same order), with y = g+ - g and d the direction just searched:
//   1. the first direction after create / reset / qn_solver_set_cg is -g (not counted as a restart);
//   2. restart_every > 0 and that many iterations since the last -g direction: beta = 0;
//   3. the variant's formula with plain IEEE divisions (a zero denominator gives inf or NaN):
//        FR  g+.g+ / g.g        PR+ max(0, g+.y / g.g)        HS+ max(0, g+.y / d.y)        DY  g+.g+ / d.y
//        HZ  max(betaN, eta_k), betaN = (g+.y - ((2 y.y) g+.d) / d.y) / d.y, eta_k = -1 / (sqrt(d.d) min(0.01, sqrt(g.g)))   (Hager and Zhang 2005)
//      (max is a comparison, a > b ? a : b, as in qn_vec_wolfe.hip.h; a NaN first operand gives the second);
//   4. beta not finite: beta = 0;
//   5. Powell's test: |g+.g| >= powell_nu g+.g+ : beta = 0 (powell_nu = +inf disables it);
//   6. the descent guard from the sums alone: unless -g+.g+ + beta (g+.d) < 0, beta = 0.
// Every beta that ends as exactly 0 counts in cg_restarts.
//
// Profiling mode, this method: t_hpass_ms = cg_dir_kernel, t_hreduce_ms = cg_accept_kernel (both O(n) streams; the one-workgroup kernels stay
// under t_ctl_ms).  Reductions, predication, 16-byte accesses, products that round twice, no atomics, no waiting between workgroups: as in
// qn_vec.hip.h.  The same bits from run to run.
#pragma once

#define QN_CG_NQ 8 // the direct sums of the accept pass, in the share buffer of the method's own: cpart[q * QN_VEC_MAXG + b]
#define QN_CGQ_GPGP 0
#define QN_CGQ_GPY 1
#define QN_CGQ_DY 2
#define QN_CGQ_GPD 3
#define QN_CGQ_YY 4
#define QN_CGQ_DD 5
#define QN_CGQ_GG 6
#define QN_CGQ_GPG 7

__global__ __launch_bounds__(QN_VEC_TPB) void cg_dir_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_NSOLVE || c->method != QN_NONLINEAR_CG) return;
    const double beta = c->cg_beta;
    const bool fresh = !c->cg_has_p || beta == 0.0; // rule 1, or a restart: d = -g without reading p
    double gm = 0.0, dm = 0.0, gd[1] = {0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d g = ld2(a.g + 2 * j);
        v2d d;
        if (fresh) {
            d.x = -g.x;
            d.y = -g.y;
        } else {
            const v2d p = ld2(a.cp + 2 * j);
            const double b0 = beta * p.x, b1 = beta * p.y; // `beta * d` rounds first
            d.x = b0 - g.x;
            d.y = b1 - g.y;
        }
        st2(a.cp + 2 * j, d);
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

// vec_accept_kernel for QN_NONLINEAR_CG.  (The machine's vec_needs_y rule has evaluated x_next: gt_valid is set whenever this runs.)
__global__ __launch_bounds__(QN_VEC_TPB) void cg_accept_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_ACCEPT || c->method != QN_NONLINEAR_CG) return;
    const double t = c->t;
    const int64_t row = (int64_t)c->n_iter;
    const bool xtr = c->trace_x && a.xtrace && row < c->trace_cap;
    double acc[2 + QN_CG_NQ];
#pragma unroll
    for (int q = 0; q < 2 + QN_CG_NQ; ++q) acc[q] = 0.0;
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), d = ld2(a.d + 2 * j);
        const v2d g = ld2(a.g + 2 * j), gt = ld2(a.gt + 2 * j);
        const double td0 = t * d.x, td1 = t * d.y;
        v2d xn;
        xn.x = x.x + td0;
        xn.y = x.y + td1;
        const double s0 = xn.x - x.x, s1 = xn.y - x.y;
        const double y0 = gt.x - g.x, y1 = gt.y - g.y;
        acc[1] = acc[1] + s0 * s0;
        acc[1] = acc[1] + s1 * s1;
        acc[0] = acc[0] + s0 * y0;
        acc[0] = acc[0] + s1 * y1;
        acc[2 + QN_CGQ_GPGP] = acc[2 + QN_CGQ_GPGP] + gt.x * gt.x;
        acc[2 + QN_CGQ_GPGP] = acc[2 + QN_CGQ_GPGP] + gt.y * gt.y;
        acc[2 + QN_CGQ_GPY] = acc[2 + QN_CGQ_GPY] + gt.x * y0;
        acc[2 + QN_CGQ_GPY] = acc[2 + QN_CGQ_GPY] + gt.y * y1;
        acc[2 + QN_CGQ_DY] = acc[2 + QN_CGQ_DY] + d.x * y0;
        acc[2 + QN_CGQ_DY] = acc[2 + QN_CGQ_DY] + d.y * y1;
        acc[2 + QN_CGQ_GPD] = acc[2 + QN_CGQ_GPD] + gt.x * d.x;
        acc[2 + QN_CGQ_GPD] = acc[2 + QN_CGQ_GPD] + gt.y * d.y;
        acc[2 + QN_CGQ_YY] = acc[2 + QN_CGQ_YY] + y0 * y0;
        acc[2 + QN_CGQ_YY] = acc[2 + QN_CGQ_YY] + y1 * y1;
        acc[2 + QN_CGQ_DD] = acc[2 + QN_CGQ_DD] + d.x * d.x;
        acc[2 + QN_CGQ_DD] = acc[2 + QN_CGQ_DD] + d.y * d.y;
        acc[2 + QN_CGQ_GG] = acc[2 + QN_CGQ_GG] + g.x * g.x;
        acc[2 + QN_CGQ_GG] = acc[2 + QN_CGQ_GG] + g.y * g.y;
        acc[2 + QN_CGQ_GPG] = acc[2 + QN_CGQ_GPG] + gt.x * g.x;
        acc[2 + QN_CGQ_GPG] = acc[2 + QN_CGQ_GPG] + gt.y * g.y;
        st2(a.g + 2 * j, gt);
        st2(a.x + 2 * j, xn);
        if (xtr) {
            if (2 * j < a.n) a.xtrace[(size_t)row * a.n + 2 * j] = xn.x;
            if (2 * j + 1 < a.n) a.xtrace[(size_t)row * a.n + 2 * j + 1] = xn.y;
        }
    }
    ctl_block_sum<2 + QN_CG_NQ>(acc, lds);
    if (threadIdx.x == 0) {
        a.part[2 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        a.part[3 * QN_VEC_MAXG + blockIdx.x] = acc[1];
#pragma unroll
        for (int q = 0; q < QN_CG_NQ; ++q) a.cpart[q * QN_VEC_MAXG + blockIdx.x] = acc[2 + q];
    }
}

// vec_post_kernel's branch, every thread: the eight sums from the method's own share buffer, in index order
__device__ __forceinline__ void cg_post_sums(const QnVecArgs& a, double* q /* [QN_CG_NQ] */, double* lds) {
#pragma unroll
    for (int i = 0; i < QN_CG_NQ; ++i) q[i] = vec_sum_parts(a.cpart, i, a.G, lds);
}

// ... and thread 0: rules 2-6 on those sums; beta, the counters and "p exists" into the control block.  Returns `updated` (beta != 0).
__device__ __forceinline__ int cg_post(QnVecCtl* c, const double* q /* [QN_CG_NQ] */) {
    const double gpgp = q[QN_CGQ_GPGP], gpy = q[QN_CGQ_GPY], dy = q[QN_CGQ_DY], gpd = q[QN_CGQ_GPD];
    const double yy = q[QN_CGQ_YY], dd = q[QN_CGQ_DD], gg = q[QN_CGQ_GG], gpg = q[QN_CGQ_GPG];
    c->cg_since++; // iterations since the last -g direction, this one included
    double beta;
    if (c->cg_restart_every > 0 && c->cg_since >= c->cg_restart_every) {
        beta = 0.0;
    } else {
        if (c->cg_variant == QN_CG_FR) {
            beta = gpgp / gg;
        } else if (c->cg_variant == QN_CG_PR_PLUS) {
            beta = wolfe_mx(gpy / gg, 0.0);
        } else if (c->cg_variant == QN_CG_HS_PLUS) {
            beta = wolfe_mx(gpy / dy, 0.0);
        } else if (c->cg_variant == QN_CG_DY) {
            beta = gpgp / dy;
        } else {
            const double two_yy = 2.0 * yy;
            const double corr = (two_yy * gpd) / dy;
            const double beta_n = (gpy - corr) / dy;
            const double eta = -1.0 / (sqrt(dd) * wolfe_mn(0.01, sqrt(gg)));
            beta = wolfe_mx(beta_n, eta);
        }
        if (isnan(beta) || isinf(beta)) beta = 0.0;
        if (fabs(gpg) >= c->cg_powell_nu * gpgp) beta = 0.0;
        const double bgd = beta * gpd;
        if (!(-gpgp + bgd < 0.0)) beta = 0.0;
    }
    if (beta == 0.0) { beta = 0.0; c->cg_restarts++; c->cg_since = 0; } // (-0.0 is stored as +0.0)
    c->cg_beta = beta;
    c->cg_has_p = 1;
    return beta != 0.0 ? 1 : 0;
}
