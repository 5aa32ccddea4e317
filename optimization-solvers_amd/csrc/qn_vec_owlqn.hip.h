// qn_vec_owlqn.hip.h -- QN_OWLQN on the first-order family's machine (qn_vec.hip.h): min f(x) + sum_j l1_j |x_j|, unbounded, by orthant-wise
// limited-memory quasi-Newton (Andrew and Gao, ICML 2007).  The curvature is QN_LBFGS's: lbfgs_gram_kernel, lbfgs_mid_kernel and
// lbfgs_apply_kernel run unchanged on a copy of QnVecArgs whose g points at the pseudo-gradient v, and the ring of pairs and its commit rule are
// vec_post_kernel's.  The rules are DESIGN.md section 35's; tests/ref_owlqn.py restates them.
//
//   owl_pg_kernel<L1VEC>     phases EVAL_X / DIR: v = prox_measure<false>(x, g, l1) per entry (rule 1); shares of ||v||_inf and h0 = h(x)
//   owl_top_kernel           (1 workgroup) two branches by phase.  EVAL_X / DIR: f_cur after an evaluation, the counters, the loop top on
//                            ||v||_inf, F_k = f_cur + h0, then QN_VP_NSOLVE.  NSOLVE (behind the direction): rule 3's test of v.d, t = 1, then
//                            QN_VP_TRIAL
//   [lbfgs_gram_kernel, lbfgs_mid_kernel, lbfgs_apply_kernel: z = H_k v]
//   owl_dir_kernel<L1VEC>    phase NSOLVE: d = -z where l1 == 0 or z and v have one sign, else 0.0 (rule 3); shares of v.d
//   owl_trial_kernel<L1VEC>  xt = the orthant projection of x + t d (rules 4, 5); in phase TRIAL the shares of h(xt) and v.(xt - x)
//   owl_decide_kernel        (1 workgroup) rule 6: F_t - F_k <= c1 v.(xt - x), or t *= beta
//   owl_accept_kernel        in lbfgs_accept_kernel's place: x_next = xt -- never x + t d --, s and y into the staging slot, shares of s.y, s.s, y.y
//   vec_post_kernel runs as it is (its lbfgs flag, vec_needs_y and vec_nsolve know the method).
//
// As in qn_vec_prox.hip.h the one-workgroup decisions are SIBLINGS launched in the existing kernels' places and QnVecCtl is untouched: h0, v.d
// and F_k are three doubles of the method's own (QnOwlArgs.pst), and f_cur stays the smooth part, so a memoised evaluation outlives a new l1.
// Shares: part 0 (max |v|) and 3 (h0) for the loop top, 1 (v.d) for the direction, 0 (h(xt)) and 1 (v.(xt - x)) for a trial, 2, 3, 5 for the accept.
// Two-stage sums in the family's fixed order, no atomics, product and sum rounded separately: the same bits from run to run.
// Entries n .. n_pad hold x = g = 0 (and l1 = 0 in the vector), so v = z = 0 there, d and xt are zeros, and no share receives anything.
#pragma once

struct QnOwlArgs {
    QnVecArgs v;
    const double* l1; // n_pad entries, zero-padded (L1VEC), or nullptr
    double l1s;       // the scalar (!L1VEC)
    double* pst;      // [0] h0, [1] v.d, [2] F_k of the iteration being searched
    double* pg;       // the pseudo-gradient v, n_pad entries
};

template <bool L1VEC>
__global__ __launch_bounds__(QN_VEC_TPB) void owl_pg_kernel(const QnOwlArgs oa) {
    __shared__ double lds[64];
    const QnVecArgs& a = oa.v;
    const QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_EVAL_X && ph != QN_VP_DIR) return;
    double mm = 0.0, h0[1] = {0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), g = ld2(a.g + 2 * j);
        v2d w, v;
        if (L1VEC) w = ld2(oa.l1 + 2 * j); else { w.x = oa.l1s; w.y = oa.l1s; }
        v.x = prox_measure<false>(x.x, g.x, w.x, 0.0, 0.0);
        v.y = prox_measure<false>(x.y, g.y, w.y, 0.0, 0.0);
        st2(oa.pg + 2 * j, v);
        mm = fmax(mm, fmax(fabs(v.x), fabs(v.y)));
        h0[0] = h0[0] + w.x * fabs(x.x);
        h0[0] = h0[0] + w.y * fabs(x.y);
    }
    mm = vec_block_max(mm, lds);
    __syncthreads();
    ctl_block_sum<1>(h0, lds);
    if (threadIdx.x == 0) {
        a.part[0 * QN_VEC_MAXG + blockIdx.x] = mm;
        a.part[3 * QN_VEC_MAXG + blockIdx.x] = h0[0];
    }
}

__global__ __launch_bounds__(QN_VEC_TPB) void owl_top_kernel(const QnOwlArgs oa) {
    __shared__ double lds[64];
    const QnVecArgs& a = oa.v;
    QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph == QN_VP_EVAL_X || ph == QN_VP_DIR) { // the loop top
        const double mm = vec_max_parts(a.part, 0, a.G, lds);
        const double h0 = vec_sum_parts(a.part, 3, a.G, lds);
        if (threadIdx.x != 0) return;
        if (ph == QN_VP_EVAL_X) { c->f_cur = *a.f_dev; c->have_eval = 1; c->n_evals++; c->ex_g_true = 1; c->ex_since = 0; }
        c->n_calls++;
        if (vec_loop_top(c, mm)) return; // out-of-domain on the smooth f, then rule 1's measure against tol
        const double fk = c->f_cur + h0;
        oa.pst[0] = h0; oa.pst[2] = fk;
        c->tr_f = fk;
        c->phase = QN_VP_NSOLVE;
        return;
    }
    if (ph != QN_VP_NSOLVE) return;
    const double vd = vec_sum_parts(a.part, 1, a.G, lds); // behind owl_dir_kernel
    if (threadIdx.x != 0) return;
    oa.pst[1] = vd;
    c->gd = vd;
    if (!(vd < 0.0) || isinf(vd)) { c->status = QN_ABNORMAL_TERMINATION; c->phase = QN_VP_DONE; return; } // rule 3: not a descent direction; x stays x_k
    c->t = 1.0;
    c->ls_i = 0;
    if (c->max_iter_ls <= 0) vec_ls_return(c, false);
    else c->phase = QN_VP_TRIAL;
}

// rule 3, one entry: comparisons, never the product's sign (a product can underflow).  The three tests are combined without short-circuit
// evaluation on purpose: one select per entry, no divergent branch in a kernel that streams memory.
__device__ __forceinline__ double owl_align(double z, double v, double w) {
    const bool keep = (w == 0.0) | ((z > 0.0) & (v > 0.0)) | ((z < 0.0) & (v < 0.0));
    return keep ? -z : 0.0;
}

template <bool L1VEC>
__global__ __launch_bounds__(QN_VEC_TPB) void owl_dir_kernel(const QnOwlArgs oa) {
    __shared__ double lds[64];
    const QnVecArgs& a = oa.v;
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_NSOLVE) return;
    double vd[1] = {0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d z = ld2(a.z + 2 * j), v = ld2(oa.pg + 2 * j);
        v2d w, d;
        if (L1VEC) w = ld2(oa.l1 + 2 * j); else { w.x = oa.l1s; w.y = oa.l1s; }
        d.x = owl_align(z.x, v.x, w.x);
        d.y = owl_align(z.y, v.y, w.y);
        st2(a.d + 2 * j, d);
        vd[0] = vd[0] + v.x * d.x;
        vd[0] = vd[0] + v.y * d.y;
    }
    ctl_block_sum<1>(vd, lds);
    if (threadIdx.x == 0) a.part[1 * QN_VEC_MAXG + blockIdx.x] = vd[0];
}

// rules 4 and 5, one entry: u = x + t d with t d rounded first; kept where the entry is smooth or u lies strictly inside the orthant of
// xi = sign(x), or sign(-v) at x == 0; otherwise the literal 0.0
__device__ __forceinline__ double owl_point(double x, double d, double v, double w, double t) {
    const double td = t * d;
    const double u = x + td;
    const bool pos = (x > 0.0) | ((x == 0.0) & (v < 0.0)), neg = (x < 0.0) | ((x == 0.0) & (v > 0.0));
    const bool keep = (w == 0.0) | ((u > 0.0) & pos) | ((u < 0.0) & neg);
    return keep ? u : 0.0;
}

template <bool L1VEC>
__global__ __launch_bounds__(QN_VEC_TPB) void owl_trial_kernel(const QnOwlArgs oa) {
    __shared__ double lds[64];
    const QnVecArgs& a = oa.v;
    const QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) return;
    const bool sums = ph == QN_VP_TRIAL; // (the re-evaluation at the accepted point is for y alone)
    const double t = c->t;
    double acc[2] = {0.0, 0.0}; // h(xt), v.(xt - x)
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), d = ld2(a.d + 2 * j), v = ld2(oa.pg + 2 * j);
        v2d w, p;
        if (L1VEC) w = ld2(oa.l1 + 2 * j); else { w.x = oa.l1s; w.y = oa.l1s; }
        p.x = owl_point(x.x, d.x, v.x, w.x, t);
        p.y = owl_point(x.y, d.y, v.y, w.y, t);
        st2(a.xt + 2 * j, p);
        if (sums) {
            acc[0] = acc[0] + w.x * fabs(p.x);
            acc[0] = acc[0] + w.y * fabs(p.y);
            const double e0 = p.x - x.x, e1 = p.y - x.y; // each difference rounded before its product
            acc[1] = acc[1] + v.x * e0;
            acc[1] = acc[1] + v.y * e1;
        }
    }
    if (!sums) return;
    ctl_block_sum<2>(acc, lds);
    if (threadIdx.x == 0) {
        a.part[0 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        a.part[1 * QN_VEC_MAXG + blockIdx.x] = acc[1];
    }
}

__global__ __launch_bounds__(QN_VEC_TPB) void owl_decide_kernel(const QnOwlArgs oa) {
    __shared__ double lds[64];
    const QnVecArgs& a = oa.v;
    QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) return;
    double hxt = 0.0, vs = 0.0;
    if (ph == QN_VP_TRIAL) {
        hxt = vec_sum_parts(a.part, 0, a.G, lds);
        vs = vec_sum_parts(a.part, 1, a.G, lds);
    }
    if (threadIdx.x != 0) return;
    const double fs = *a.f_dev;
    c->f_t = fs; // the smooth part: what the post kernel makes f_cur
    c->n_calls++; c->n_evals++; c->tr_n_evals++;
    if (ph == QN_VP_REEVAL) { c->gt_valid = 1; c->phase = QN_VP_ACCEPT; return; }
    c->tr_ls_iters++;
    const double ft = fs + hxt;
    const double t = c->t, fk = oa.pst[2];
    if (isnan(ft) || isinf(ft)) { // a non-finite trial shrinks without counting
        c->t = t * c->beta;
        return;
    }
    if (ft - fk <= c->c1 * vs) { vec_ls_return(c, true); return; } // Andrew and Gao's condition: no factor t, the projected step is not t d
    c->t = t * c->beta;
    c->ls_i++;
    if (c->ls_i >= c->max_iter_ls) vec_ls_return(c, false);
}

// lbfgs_accept_kernel for QN_OWLQN: x_next = xt, the projected point the trial kernel formed last (the accepted trial, or the same arithmetic again
// in phase REEVAL); s = x_next - x, y = g(x_next) - g(x) -- the smooth gradients -- into the staging slot, with the shares of s.y, s.s and y.y
__global__ __launch_bounds__(QN_VEC_TPB) void owl_accept_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_ACCEPT) return;
    const int64_t row = (int64_t)c->n_iter;
    const bool xtr = c->trace_x && a.xtrace && row < c->trace_cap;
    const int M = c->lb_m + 1;
    const size_t stage = (size_t)((c->lb_head + c->lb_kmem) % M) * (size_t)a.np;
    double* Ss = a.lS + stage;
    double* Ys = a.lY + stage;
    double acc[3] = {0.0, 0.0, 0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), xn = ld2(a.xt + 2 * j);
        const v2d g = ld2(a.g + 2 * j), gt = ld2(a.gt + 2 * j);
        v2d s, y;
        s.x = xn.x - x.x; s.y = xn.y - x.y;
        y.x = gt.x - g.x; y.y = gt.y - g.y;
        acc[1] = acc[1] + s.x * s.x;
        acc[1] = acc[1] + s.y * s.y;
        acc[0] = acc[0] + s.x * y.x;
        acc[0] = acc[0] + s.y * y.y;
        acc[2] = acc[2] + y.x * y.x;
        acc[2] = acc[2] + y.y * y.y;
        st2(Ss + 2 * j, s);
        st2(Ys + 2 * j, y);
        st2(a.g + 2 * j, gt);
        st2(a.x + 2 * j, xn);
        if (xtr) {
            if (2 * j < a.n) a.xtrace[(size_t)row * a.n + 2 * j] = xn.x;
            if (2 * j + 1 < a.n) a.xtrace[(size_t)row * a.n + 2 * j + 1] = xn.y;
        }
    }
    ctl_block_sum<3>(acc, lds);
    if (threadIdx.x == 0) {
        a.part[2 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        a.part[3 * QN_VEC_MAXG + blockIdx.x] = acc[1];
        a.part[5 * QN_VEC_MAXG + blockIdx.x] = acc[2];
    }
}
