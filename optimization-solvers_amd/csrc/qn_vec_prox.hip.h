// qn_vec_prox.hip.h -- QN_SPECTRAL_PROXIMAL_GRADIENT on the first-order family's machine (qn_vec.hip.h): min f(x) + sum_j l1_j |x_j| in a box, by
// SPG with the projection replaced by the proximal map of lambda l1 |.| plus the box (SpaRSA: Wright, Nowak, Figueiredo 2009), the composite
// decrease of Tseng and Yun in the non-monotone search.  The rules are DESIGN.md section 34's; tests/ref_prox.py restates them.
//
//   prox_dir_kernel<BOXED, L1VEC>   in vec_dir_kernel's place: d = clip(soft(x - lambda g, lambda l1)) - x; shares of the measure, g.d, ||d||_inf,
//                                   h0 = h(x) and h1 = h(x + d)
//   prox_top_kernel                 (1 workgroup) in vec_top_kernel's place: lambda0, out-of-domain, convergence on rule 2's measure,
//                                   Delta = g.d + (h1 - h0), F_k = f_cur + h0 into the ring, the first trial t = 1
//   prox_trial_kernel<L1VEC>        in vec_trial_kernel's place: xt = x + t d; in phase QN_VP_TRIAL the shares of h(xt)
//   prox_decide_kernel              (1 workgroup) in vec_decide_kernel's place: vec_decide_kernel's GLLQuadratic and Armijo branches on
//                                   F_t = f(xt) + h(xt), F_k and Delta
//   vec_accept_kernel, vec_post_kernel run as they are (vec_spectral and vec_needs_y know the method).
//
// The one-workgroup decisions are SIBLINGS launched in the existing kernels' places, not branches inside them: no instruction of another
// method's kernels changes.  QnVecCtl is untouched as well: the scalars that live from the loop top to the search's last trial (h0, Delta,
// F_k) are three doubles of the method's own (QnProxArgs.pst), and f_cur stays the smooth part, so a memoised evaluation outlives a new l1.
// Shares: parts 0 .. 4 of the family's buffer for a direction batch (3 .. 5 are free while the direction runs), part 0 for a trial.
// Two-stage sums in the family's fixed order, no atomics, product and sum rounded separately: the same bits from run to run.
// Entries n .. n_pad hold x = g = d = 0 (and l1 = 0 in the vector): they add nothing to any share, with a scalar l1 as well (l1 |0| = 0,
// soft(0, tau) = 0, and 0 lies in [g - l1, g + l1]).
#pragma once

struct QnProxArgs {
    QnVecArgs v;
    const double* l1; // n_pad entries, zero-padded (L1VEC), or nullptr
    double l1s;       // the scalar (!L1VEC)
    double* pst;      // [0] h0, [1] Delta, [2] F_k of the iteration being searched
};

// rule 1, one entry: sg, u, tau, the soft threshold, the clip, the difference -- six roundings at the most, in this order
template <bool BOXED>
__device__ __forceinline__ double prox_entry(double x, double g, double lam, double l1, double lo, double hi) {
    const double sg = lam * g;
    const double u = x - sg;
    const double tau = lam * l1;
    double z = 0.0;
    if (u > tau) z = u - tau;
    else if (u < -tau) z = u + tau;
    const double p = BOXED ? fmin(fmax(z, lo), hi) : z;
    return p - x;
}
// rule 2, one entry: the element of least magnitude of the subdifferential's interval, opened towards the side a bound blocks
template <bool BOXED>
__device__ __forceinline__ double prox_measure(double x, double g, double l1, double lo, double hi) {
    double a = x > 0.0 ? g + l1 : g - l1;
    double b = x < 0.0 ? g - l1 : g + l1;
    if (BOXED) {
        if (x == lo) a = -INFINITY;
        if (x == hi) b = INFINITY;
    }
    return a > 0.0 ? a : (b < 0.0 ? b : 0.0);
}

template <bool BOXED, bool L1VEC>
__global__ __launch_bounds__(QN_VEC_TPB) void prox_dir_kernel(const QnProxArgs pa) {
    __shared__ double lds[64];
    const QnVecArgs& a = pa.v;
    const QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_EVAL_X && ph != QN_VP_DIR && ph != QN_VP_LS_ONLY && ph != QN_VP_NSOLVE) return; // (vec_dir_kernel's predicate; the last two never occur here)
    const double lam = c->has_lambda ? c->lambda : 1.0; // before lambda exists it counts as 1: 1 * g is g
    double mm = 0.0, dm = 0.0, acc[3] = {0.0, 0.0, 0.0}; // g.d, h0, h1
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), g = ld2(a.g + 2 * j);
        v2d w, lo, hi;
        if (L1VEC) w = ld2(pa.l1 + 2 * j); else { w.x = pa.l1s; w.y = pa.l1s; }
        if (BOXED) { lo = ld2(a.lb + 2 * j); hi = ld2(a.ub + 2 * j); } else { lo.x = lo.y = -INFINITY; hi.x = hi.y = INFINITY; }
        v2d d;
        d.x = prox_entry<BOXED>(x.x, g.x, lam, w.x, lo.x, hi.x);
        d.y = prox_entry<BOXED>(x.y, g.y, lam, w.y, lo.y, hi.y);
        st2(a.d + 2 * j, d);
        const double m0 = prox_measure<BOXED>(x.x, g.x, w.x, lo.x, hi.x), m1 = prox_measure<BOXED>(x.y, g.y, w.y, lo.y, hi.y);
        mm = fmax(mm, fmax(fabs(m0), fabs(m1)));
        dm = fmax(dm, fmax(fabs(d.x), fabs(d.y)));
        acc[0] = acc[0] + g.x * d.x;
        acc[0] = acc[0] + g.y * d.y;
        acc[1] = acc[1] + w.x * fabs(x.x);
        acc[1] = acc[1] + w.y * fabs(x.y);
        const double e0 = x.x + d.x, e1 = x.y + d.y; // the trial kernel's x + 1 * d
        acc[2] = acc[2] + w.x * fabs(e0);
        acc[2] = acc[2] + w.y * fabs(e1);
    }
    mm = vec_block_max(mm, lds);
    __syncthreads();
    dm = vec_block_max(dm, lds);
    __syncthreads();
    ctl_block_sum<3>(acc, lds);
    if (threadIdx.x == 0) {
        a.part[0 * QN_VEC_MAXG + blockIdx.x] = mm;
        a.part[1 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        a.part[2 * QN_VEC_MAXG + blockIdx.x] = dm;
        a.part[3 * QN_VEC_MAXG + blockIdx.x] = acc[1];
        a.part[4 * QN_VEC_MAXG + blockIdx.x] = acc[2];
    }
}

__global__ __launch_bounds__(QN_VEC_TPB) void prox_top_kernel(const QnProxArgs pa) {
    __shared__ double lds[64];
    const QnVecArgs& a = pa.v;
    QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_EVAL_X && ph != QN_VP_DIR) return;
    const double mm = vec_max_parts(a.part, 0, a.G, lds);
    const double gd = vec_sum_parts(a.part, 1, a.G, lds);
    const double dm = vec_max_parts(a.part, 2, a.G, lds);
    const double h0 = vec_sum_parts(a.part, 3, a.G, lds);
    const double h1 = vec_sum_parts(a.part, 4, a.G, lds);
    if (threadIdx.x != 0) return;
    if (ph == QN_VP_EVAL_X) { c->f_cur = *a.f_dev; c->have_eval = 1; c->n_evals++; c->ex_g_true = 1; c->ex_since = 0; }
    c->n_calls++;
    if (!c->has_lambda) { // the constructor's call: d was formed with lambda = 1 (spg.rs:40-46 with the prox in the projection's place)
        c->lambda = fmax(fmin(1.0 / dm, c->lambda_max), c->lambda_min);
        c->has_lambda = 1;
        if (c->max_iter <= 0) { c->status = QN_MAX_ITER_REACHED; c->phase = QN_VP_DONE; return; }
        c->phase = c->memoize ? QN_VP_DIR : QN_VP_EVAL_X;
        return;
    }
    if (vec_loop_top(c, mm)) return; // out-of-domain on the smooth f, then rule 2's measure against tol
    const double hd = h1 - h0;
    const double delta = gd + hd; // Tseng and Yun's composite decrease; no test of its sign
    const double fk = c->f_cur + h0;
    pa.pst[0] = h0; pa.pst[1] = delta; pa.pst[2] = fk;
    c->tr_f = fk;
    c->gd = delta;
    if (c->ls_kind == QN_LS_GLL_QUADRATIC) { // the ring holds composite values
        if (c->ring_len == c->m) {
            for (int i = 1; i < c->ring_len; ++i) c->ring[i - 1] = c->ring[i];
            c->ring_len--;
        }
        c->ring[c->ring_len++] = fk;
        double fm = -INFINITY;
        for (int i = 0; i < c->ring_len; ++i) fm = fmax(c->ring[i], fm);
        c->f_max = fm;
    }
    c->t = 1.0;
    c->ls_i = 0;
    if (c->max_iter_ls <= 0) vec_ls_return(c, false);
    else c->phase = QN_VP_TRIAL;
}

template <bool L1VEC>
__global__ __launch_bounds__(QN_VEC_TPB) void prox_trial_kernel(const QnProxArgs pa) {
    __shared__ double lds[64];
    const QnVecArgs& a = pa.v;
    const QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) return;
    const bool pen = ph == QN_VP_TRIAL; // (the re-evaluation at the accepted point is for y alone)
    const double t = c->t;
    double ht[1] = {0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), d = ld2(a.d + 2 * j);
        const double td0 = t * d.x, td1 = t * d.y; // `t * direction_k` rounds first
        v2d u;
        u.x = x.x + td0;
        u.y = x.y + td1;
        st2(a.xt + 2 * j, u);
        if (pen) {
            v2d w;
            if (L1VEC) w = ld2(pa.l1 + 2 * j); else { w.x = pa.l1s; w.y = pa.l1s; }
            ht[0] = ht[0] + w.x * fabs(u.x);
            ht[0] = ht[0] + w.y * fabs(u.y);
        }
    }
    if (!pen) return;
    ctl_block_sum<1>(ht, lds);
    if (threadIdx.x == 0) a.part[0 * QN_VEC_MAXG + blockIdx.x] = ht[0];
}

__global__ __launch_bounds__(QN_VEC_TPB) void prox_decide_kernel(const QnProxArgs pa) {
    __shared__ double lds[64];
    const QnVecArgs& a = pa.v;
    QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) return;
    double hxt = 0.0;
    if (ph == QN_VP_TRIAL) hxt = vec_sum_parts(a.part, 0, a.G, lds);
    if (threadIdx.x != 0) return;
    const double fs = *a.f_dev;
    c->f_t = fs; // the smooth part: what the post kernel makes f_cur
    c->n_calls++; c->n_evals++; c->tr_n_evals++;
    if (ph == QN_VP_REEVAL) { c->gt_valid = 1; c->phase = QN_VP_ACCEPT; return; }
    c->tr_ls_iters++;
    const double ft = fs + hxt;
    const double t = c->t, gd = pa.pst[1], fk = pa.pst[2];
    if (c->ls_kind == QN_LS_GLL_QUADRATIC) {
        if (ft - c->f_max <= c->c1 * t * gd) { vec_ls_return(c, true); return; }
        if (t <= 0.1) {
            c->t = t * 0.5;
        } else {
            const double t_tmp = -0.5 * t * t * gd / (ft - fk - t * gd);
            if (t_tmp > c->sigma1 && t_tmp < c->sigma2 * t) c->t = t_tmp;
            else c->t = t_tmp * 0.5;
        }
        c->ls_i++;
    } else { // QN_LS_BACKTRACKING
        if (isnan(ft) || isinf(ft)) { // a non-finite trial shrinks without counting
            c->t = t * c->beta;
            return;
        }
        if (ft - fk <= c->c1 * t * gd) { vec_ls_return(c, true); return; }
        c->t = t * c->beta;
        c->ls_i++;
    }
    if (c->ls_i >= c->max_iter_ls) vec_ls_return(c, false);
}
