// qn_vec_wolfe.hip.h -- the StrongWolfe line search (QN_LS_STRONG_WOLFE) of the first-order family's machine (qn_vec.hip.h): MINPACK-2 `dcsrch` /
// `dcstep` (More' and Thuente, ACM TOMS 20, 1994) with ONE oracle call per trial and the bracket's (f, f') kept in the control block.  (NOT
// the reference's transcription, line_search/morethuente.rs:181-294, which calls the oracle two or three times per inner iteration: here an oracle
// call is a device-wide stream, or a full pass over Q or A.)
//
//   wolfe_clip_kernel    boxed form only, behind every vec_dir_kernel: one stream of x, d, llb, lub -> partial minima of the ratio of
//                        morethuente_b.rs:185-197 ((ub_i - x_i) / d_i, (lb_i - x_i) / d_i, +inf for d_i = 0; the fold starts from +inf)
//   [vec_top_kernel]     its branch for this kind (wolfe_start): stpmax = min(t_max, the clip) for THIS search, dcsrch's START, the first trial
//   [vec_trial_kernel]   xt = x + t d, as for every kind
//   [the oracle at xt]
//   wolfe_phi_kernel     partials of phi'(t) = gt . d: one stream of gt and d, 16 n bytes -- the only per-trial stream this search adds
//   wolfe_decide_kernel  (1 workgroup, in vec_decide_kernel's place) one dcsrch step by thread 0: the tests, the stage switch, dcstep's four
//                        cases, the bracket update, the safeguarded bisection -> vec_ls_return, or the next t with phase QN_VP_TRIAL
//
// ftol = c1, gtol = c2, xtol, stpmin = t_min, stpmax = t_max; the first trial is min(max(1, stpmin), stpmax).  The search ends on the strong-Wolfe
// test, on stp = stpmax with sufficient decrease and a derivative <= ftol g.d, on stp = stpmin, on the xtol test and on the rounding-error test:
// in every one of these the returned step is the one just evaluated ((f_t, gt) are valid: vec_ls_return(c, true)).  Running out of
// max_iter_line_search returns the NEXT step, unevaluated, as this family's other searches do.
//
// TWO RULES dcsrch DOES NOT HAVE.
//   * A trial whose f (or phi') is not finite counts as "sufficient decrease fails, derivative positive": no test that needs f passes (stp = stpmin
//     still ends the search), the bracket becomes [stx, stp] and the next trial bisects it.  The end point keeps fy = +inf, and the one dcstep case
//     that interpolates through the far end point (case 4, bracketed) bisects [stp, sty] instead while that is so.  Trace digit 5.
//   * g.d >= 0 (or NaN) at the start -- dcsrch's "ERROR: INITIAL G .GE. ZERO" -- and stpmax < stpmin end the run with QN_ABNORMAL_TERMINATION
//     ("not a descent direction"); x stays at x_k.  ProjectedLBFGS with an active box can meet it: d = P(x - H g) - x need not descend.
//
// max / min / clip are comparisons (a > b ? a : b), written the same way in tests/ref_wolfe.py.  Reductions, predication, 16-byte accesses, products
// that round twice, no atomics, no waiting between workgroups: as in qn_vec.hip.h.  The same bits from run to run.
#pragma once

#define QN_WP_CLIP 6 // shares of part[][]: the ratio's minima
#define QN_WP_PHI 7  //                     gt . d

__device__ __forceinline__ double wolfe_min_parts(const double* part, int q, int G, double* lds) {
    double v = INFINITY;
    for (int b = threadIdx.x; b < G; b += QN_VEC_TPB) v = fmin(part[q * QN_VEC_MAXG + b], v);
    __syncthreads();
    return -vec_block_max(-v, lds);
}

__global__ __launch_bounds__(QN_VEC_TPB) void wolfe_clip_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_EVAL_X && ph != QN_VP_DIR && ph != QN_VP_NSOLVE) return;
    if (c->ls_kind != QN_LS_STRONG_WOLFE || !c->w_boxed) return;
    double m = INFINITY;
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), d = ld2(a.d + 2 * j), lo = ld2(a.llb + 2 * j), hi = ld2(a.lub + 2 * j);
        const double r0 = d.x > 0.0 ? (hi.x - x.x) / d.x : (d.x < 0.0 ? (lo.x - x.x) / d.x : INFINITY);
        const double r1 = d.y > 0.0 ? (hi.y - x.y) / d.y : (d.y < 0.0 ? (lo.y - x.y) / d.y : INFINITY);
        m = fmin(r0, m);
        m = fmin(r1, m);
    }
    m = -vec_block_max(-m, lds);
    if (threadIdx.x == 0) a.part[QN_WP_CLIP * QN_VEC_MAXG + blockIdx.x] = m;
}

__global__ __launch_bounds__(QN_VEC_TPB) void wolfe_phi_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_TRIAL || c->ls_kind != QN_LS_STRONG_WOLFE) return;
    double acc[1] = {0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d g = ld2(a.gt + 2 * j), d = ld2(a.d + 2 * j);
        acc[0] = acc[0] + g.x * d.x;
        acc[0] = acc[0] + g.y * d.y;
    }
    ctl_block_sum<1>(acc, lds);
    if (threadIdx.x == 0) a.part[QN_WP_PHI * QN_VEC_MAXG + blockIdx.x] = acc[0];
}

__device__ __forceinline__ double wolfe_mx(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double wolfe_mn(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ void wolfe_push_case(QnVecCtl* c, int digit) { // tr_push_case of the dense path
    if (c->tr_ndigits < 10) {
        int32_t mul = 1;
        for (int i = 0; i < c->tr_ndigits; ++i) mul *= 8;
        c->tr_ls_cases += mul * digit;
    }
    c->tr_ndigits++;
}

// vec_top_kernel's branch (thread 0): dcsrch's START for the search that opens here.  false: the run has ended.
__device__ __forceinline__ bool wolfe_start(QnVecCtl* c, double gd, double clip) {
    const double stpmin = c->w_tmin;
    const double stpmax = c->w_boxed ? fmin(c->w_tmax, clip) : c->w_tmax; // per search: never written back into the line-search value
    c->w_stpmax = stpmax;
    if (!(gd < 0.0)) { c->w_err = 1; c->status = QN_ABNORMAL_TERMINATION; c->phase = QN_VP_DONE; return false; }
    if (stpmax < stpmin) { c->w_err = 2; c->status = QN_ABNORMAL_TERMINATION; c->phase = QN_VP_DONE; return false; }
    c->w_brackt = 0; c->w_stage = 1;
    c->w_finit = c->f_cur; c->w_ginit = gd;
    c->w_gtest = c->c1 * gd;
    c->w_width = stpmax - stpmin;
    c->w_width1 = c->w_width / 0.5;
    c->w_stx = 0.0; c->w_fx = c->f_cur; c->w_gx = gd;
    c->w_sty = 0.0; c->w_fy = c->f_cur; c->w_gy = gd;
    const double stp = wolfe_mn(wolfe_mx(1.0, stpmin), stpmax);
    c->w_stmin = 0.0;
    c->w_stmax = stp + 4.0 * stp;
    c->t = stp;
    return true;
}

// dcstep: the safeguarded step and the interval update; returns the case (1 .. 4)
__device__ __forceinline__ int wolfe_dcstep(double& stx, double& fx, double& dx, double& sty, double& fy, double& dy, double& stp, const double fp,
                                            const double dp, int& brackt, const double stpmin, const double stpmax) {
    const double sgnd = ((dp > 0.0 ? 1.0 : 0.0) - (dp < 0.0 ? 1.0 : 0.0)) * ((dx > 0.0 ? 1.0 : 0.0) - (dx < 0.0 ? 1.0 : 0.0));
    double stpf;
    int kase;
    if (fp > fx) {
        kase = 1;
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = wolfe_mx(wolfe_mx(fabs(theta), fabs(dx)), fabs(dp));
        double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
        if (stp < stx) gamma = -gamma;
        const double p = (gamma - dx) + theta;
        const double q = ((gamma - dx) + gamma) + dp;
        const double r = p / q;
        const double stpc = stx + r * (stp - stx);
        const double stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
        stpf = fabs(stpc - stx) <= fabs(stpq - stx) ? stpc : stpc + (stpq - stpc) / 2.0;
        brackt = 1;
    } else if (sgnd < 0.0) {
        kase = 2;
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = wolfe_mx(wolfe_mx(fabs(theta), fabs(dx)), fabs(dp));
        double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
        if (stp > stx) gamma = -gamma;
        const double p = (gamma - dp) + theta;
        const double q = ((gamma - dp) + gamma) + dx;
        const double r = p / q;
        const double stpc = stp + r * (stx - stp);
        const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
        stpf = fabs(stpc - stp) > fabs(stpq - stp) ? stpc : stpq;
        brackt = 1;
    } else if (fabs(dp) < fabs(dx)) {
        kase = 3;
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = wolfe_mx(wolfe_mx(fabs(theta), fabs(dx)), fabs(dp));
        const double v = (theta / s) * (theta / s) - (dx / s) * (dp / s);
        double gamma = s * sqrt(v > 0.0 ? v : 0.0);
        if (stp > stx) gamma = -gamma;
        const double p = (gamma - dp) + theta;
        const double q = (gamma + (dx - dp)) + gamma;
        const double r = p / q;
        double stpc;
        if (r < 0.0 && gamma != 0.0) stpc = stp + r * (stx - stp);
        else if (stp > stx) stpc = stpmax;
        else stpc = stpmin;
        const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
        if (brackt) {
            stpf = fabs(stpc - stp) < fabs(stpq - stp) ? stpc : stpq;
            const double lim = stp + 0.66 * (sty - stp);
            stpf = stp > stx ? wolfe_mn(lim, stpf) : wolfe_mx(lim, stpf);
        } else {
            stpf = fabs(stpc - stp) > fabs(stpq - stp) ? stpc : stpq;
            stpf = wolfe_mn(stpmax, stpf);
            stpf = wolfe_mx(stpmin, stpf);
        }
    } else {
        kase = 4;
        if (brackt) {
            if (!isnan(fy) && !isinf(fy)) {
                const double theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp;
                const double s = wolfe_mx(wolfe_mx(fabs(theta), fabs(dy)), fabs(dp));
                double gamma = s * sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s));
                if (stp > sty) gamma = -gamma;
                const double p = (gamma - dp) + theta;
                const double q = ((gamma - dp) + gamma) + dy;
                const double r = p / q;
                stpf = stp + r * (sty - stp);
            } else { // (the far end point was a non-finite trial: no cubic through it)
                stpf = stp + 0.5 * (sty - stp);
            }
        } else if (stp > stx) {
            stpf = stpmax;
        } else {
            stpf = stpmin;
        }
    }
    if (fp > fx) {
        sty = stp; fy = fp; dy = dp;
    } else {
        if (sgnd < 0.0) { sty = stx; fy = fx; dy = dx; }
        stx = stp; fx = fp; dx = dp;
    }
    stp = stpf;
    return kase;
}

__global__ __launch_bounds__(QN_VEC_TPB) void wolfe_decide_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) return;
    double g = 0.0;
    if (ph == QN_VP_TRIAL) g = vec_sum_parts(a.part, QN_WP_PHI, a.G, lds);
    if (threadIdx.x != 0) return;
    const double f = *a.f_dev;
    c->f_t = f;
    c->n_calls++; c->n_evals++; c->tr_n_evals++;
    if (ph == QN_VP_REEVAL) { c->gt_valid = 1; c->phase = QN_VP_ACCEPT; return; }
    c->tr_ls_iters++;
    double stp = c->t;
    const double stpmin = c->w_tmin, stpmax = c->w_stpmax, gtest = c->w_gtest, xtol = c->w_xtol;
    const bool bad = isnan(f) || isinf(f) || isnan(g) || isinf(g);
    const double ftest = c->w_finit + stp * gtest;
    if (c->w_stage == 1 && !bad && f <= ftest && g >= 0.0) { c->w_stage = 2; c->tr_ls_cases |= QN_TRACE_LS_MODIFIED; }
    int brackt = c->w_brackt;
    bool ended = false;
    if (brackt && (stp <= c->w_stmin || stp >= c->w_stmax)) ended = true;              // rounding errors prevent progress
    if (brackt && c->w_stmax - c->w_stmin <= xtol * c->w_stmax) ended = true;          // the xtol test
    if (!bad && stp == stpmax && f <= ftest && g <= gtest) ended = true;               // stp = stpmax
    if (stp == stpmin && (bad || f > ftest || g >= gtest)) ended = true;               // stp = stpmin
    if (!bad && f <= ftest && fabs(g) <= c->w_c2 * (-c->w_ginit)) ended = true;        // the strong-Wolfe conditions
    if (ended) { wolfe_push_case(c, 0); vec_ls_return(c, true); return; }
    double stx = c->w_stx, fx = c->w_fx, gx = c->w_gx, sty = c->w_sty, fy = c->w_fy, gy = c->w_gy;
    if (bad) {
        wolfe_push_case(c, 5);
        brackt = 1;
        sty = stp; fy = INFINITY; gy = -c->w_ginit;
        stp = stx + 0.5 * (stp - stx);
    } else if (c->w_stage == 1 && f <= fx && f > ftest) { // the modified function psi(t) = phi(t) - phi(0) - ftol phi'(0) t
        const double fm = f - stp * gtest;
        double fxm = fx - stx * gtest, fym = fy - sty * gtest;
        const double gm = g - gtest;
        double gxm = gx - gtest, gym = gy - gtest;
        wolfe_push_case(c, wolfe_dcstep(stx, fxm, gxm, sty, fym, gym, stp, fm, gm, brackt, c->w_stmin, c->w_stmax));
        fx = fxm + stx * gtest; fy = fym + sty * gtest;
        gx = gxm + gtest; gy = gym + gtest;
    } else {
        wolfe_push_case(c, wolfe_dcstep(stx, fx, gx, sty, fy, gy, stp, f, g, brackt, c->w_stmin, c->w_stmax));
    }
    if (brackt) {
        if (fabs(sty - stx) >= 0.66 * c->w_width1) stp = stx + 0.5 * (sty - stx);
        c->w_width1 = c->w_width;
        c->w_width = fabs(sty - stx);
        c->w_stmin = wolfe_mn(stx, sty);
        c->w_stmax = wolfe_mx(stx, sty);
    } else {
        c->w_stmin = stp + 1.1 * (stp - stx);
        c->w_stmax = stp + 4.0 * (stp - stx);
    }
    stp = wolfe_mx(stp, stpmin);
    stp = wolfe_mn(stp, stpmax);
    if ((brackt && (stp <= c->w_stmin || stp >= c->w_stmax)) || (brackt && c->w_stmax - c->w_stmin <= xtol * c->w_stmax)) stp = stx;
    c->w_stx = stx; c->w_fx = fx; c->w_gx = gx; c->w_sty = sty; c->w_fy = fy; c->w_gy = gy; c->w_brackt = brackt;
    c->t = stp;
    c->ls_i++;
    if (c->ls_i >= c->max_iter_ls) vec_ls_return(c, false); // "Max iter reached. Early stopping.": t was never evaluated
}
