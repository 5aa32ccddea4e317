// qn_vec.hip.h -- the first-order family: SpectralProjectedGradient (steepest_descent/spg.rs), ProjectedGradientDescent
// (steepest_descent/projected_gradient_descent.rs) and the GLLQuadratic line search (line_search/gll_quadratic.rs), with BackTracking and
// BackTrackingB beside it.  These solvers keep O(n) state, so the vectors ARE the problem: every O(n) operation runs on a device-wide grid
// with 16-byte accesses, and every decision is taken by a one-workgroup kernel from per-workgroup partials.
//
//   vec_dir_kernel     x, g, lb, ub, lambda -> d = P(x - lambda g) - x; partials ||pg||_inf, g.d, ||d||_inf
//   vec_top_kernel     (1 workgroup) loop top of ls_solver.rs:78-90: lambda0, out-of-domain, convergence, opens the line search
//   vec_trial_kernel   xt = x + t d (projected onto the line search's box for BackTrackingB: partials ||xt - x||^2, "projection moved it")
//   [the oracle at xt, enqueued by the host pump]
//   vec_decide_kernel  (1 workgroup) the line search's decision: accept, or the next t
//   vec_accept_kernel  predicated on the accept: x_next = x + t d, s, y, partials s.y, s.s; x <- x_next, g <- gt
//   vec_post_kernel    (1 workgroup) the Barzilai-Borwein scalar, the trace record, k += 1, the iteration cap
// (QN_LS_STRONG_WOLFE: wolfe_clip_kernel behind vec_dir_kernel, wolfe_phi_kernel behind the oracle, wolfe_decide_kernel in vec_decide_kernel's place:
// qn_vec_wolfe.hip.h.  QN_NONLINEAR_CG: cg_dir_kernel in phase QN_VP_NSOLVE, cg_accept_kernel in vec_accept_kernel's place: qn_cg.hip.h)
//
// REDUCTIONS are two-stage and fixed: workgroup b leaves its share in part[q * QN_VEC_MAXG + b]; the one-workgroup kernels add the G
// shares in index order (thread j takes b = j, j + 256, ..., then the block sum in wave order).  The grid is a function of n alone, no
// floating-point atomic is used, and no kernel waits for another workgroup: the same bits from run to run.
// Every kernel is predicated on QnVecCtl.phase, so the host enqueues a whole iteration without reading a decision.
// The dot products multiply and add with two roundings, as the reference does (no FMA: these kernels are bound by memory, and at n = 2 --
// the reference's own tests -- the sums then ARE the reference's, bit for bit).
#pragma once
#include <float.h>

#define QN_VEC_TPB 256
#define QN_VEC_MAXG 1024 // 4 workgroups per CU on 256 CUs
#define QN_VEC_NPART 8 // (4, 5: the second-order variants' accept kernel -- ||pg(x_next)||_inf and y.y; 6, 7: StrongWolfe's clip and phi', qn_vec_wolfe.hip.h)
#define QN_GLL_MAX_M 64

enum QnVecPhase : int32_t {
    QN_VP_IDLE = 0,
    QN_VP_EVAL_X = 1, // the oracle at x (loop top, ls_solver.rs:79; SPG's constructor, spg.rs:40), then as QN_VP_DIR
    QN_VP_DIR = 2,    // (f_cur, g) hold the evaluation at x: direction, loop top, first trial
    QN_VP_TRIAL = 3,  // the line search wants the oracle at x + t d
    QN_VP_REEVAL = 4, // SPG's update wants the oracle at x_next = x + t d, which no trial evaluated (spg.rs:130)
    QN_VP_ACCEPT = 5, // the step is decided: accept and post kernels
    QN_VP_LS_ONLY = 6, // qn_compute_step_len: g.d for the caller's direction, then the line search alone
    QN_VP_DONE = 7,
    QN_VP_NSOLVE = 8, // ProjectedNewton / SpectralProjectedNewton: the loop top let the iteration through; the host enqueues z = H^-1 g, then the direction
                      // (QN_LBFGS: z = H_k g from the last pairs (s, y), qn_lbfgs.hip.h; QN_NONLINEAR_CG: d = beta p - g written directly, qn_cg.hip.h)
    QN_VP_EXACT = 9,  // QN_LS_EXACT_QUADRATIC: the loop top left g.d < 0; the curvature pass and exact_step_kernel act (qn_vec_exact.hip.h)
    QN_VP_EXACT_REFRESH = 10 // ... the loop top's test passed on a recurrence gradient: NO kernel acts on this phase (the L-BFGS and CG batches launch
                             // vec_top_kernel a second time); the host turns it into QN_VP_EVAL_X in front of the next batch
};

// the second-order variants (newton/projected_newton.rs, newton/spn.rs): the same machine, with z = H^-1 g where the first-order family has g
__device__ __forceinline__ bool vec_newton(int method) { return method == QN_PROJECTED_NEWTON || method == QN_SPECTRAL_PROJECTED_NEWTON; }
__device__ __forceinline__ bool vec_spectral(int method) { return method == QN_SPG || method == QN_SPECTRAL_PROJECTED_NEWTON || method == QN_SPECTRAL_PROXIMAL_GRADIENT; }
// update_next_iterate calls the oracle at the accepted point, for y (spg.rs:130, spn.rs:135, projected_newton.rs:134)
__device__ __forceinline__ bool vec_needs_y(int method) { return vec_spectral(method) || method == QN_PROJECTED_NEWTON || method == QN_LBFGS || method == QN_NONLINEAR_CG || method == QN_OWLQN; }
// the direction is P(x - z) - x with a z that arrives from outside this file, in phase QN_VP_NSOLVE (QN_NONLINEAR_CG: the direction itself does)
__device__ __forceinline__ bool vec_nsolve(int method) { return vec_newton(method) || method == QN_LBFGS || method == QN_NONLINEAR_CG || method == QN_NEWTON_CG || method == QN_OWLQN; }

struct QnVecCtl {
    // ---- configuration (host, per call) ----
    double tol;
    int64_t max_iter, max_iter_ls;
    int32_t method, ls_kind, memoize, ls_only;
    double c1, beta, sigma1, sigma2;
    int32_t m, trace_x;
    int64_t trace_cap;
    double lambda_min, lambda_max;
    // ---- state that survives calls ----
    double lambda;
    int32_t has_lambda, have_eval; // have_eval: (f_cur, g) are the evaluation at x
    double f_cur;
    double ring[QN_GLL_MAX_M]; // GLLQuadratic.f_previous (gll_quadratic.rs:7), oldest first
    int32_t ring_len, _pad0;
    // ---- run state ----
    int32_t phase, status;
    int64_t k, ls_i;
    double gd, pgnorm, t, f_max, f_t, ls_result;
    int32_t gt_valid, _pad1; // (f_t, gt) are the evaluation at x + t d exactly
    // ---- per-iteration trace scratch ----
    double tr_f, tr_gnorm;
    int32_t tr_n_evals, tr_ls_iters;
    // ---- counters of this call ----
    uint64_t n_calls, n_evals, n_iter;
    // ---- ProjectedNewton: s_norm / y_norm (projected_newton.rs:10-11; survive calls, None after ::new) ----
    double s_norm, y_norm;
    int32_t has_sy, _pad2;
    // ---- QN_LBFGS (qn_lbfgs.hip.h): the memory's bookkeeping; survives calls like lambda ----
    int32_t lb_m, lb_unit;    // pairs kept at most; QN_OPT_LBFGS_UNIT_SCALING
    int32_t lb_kmem, lb_head; // live pairs, slot of the oldest (the ring has lb_m + 1 slots)
    double lb_gamma;          // the scaling of the last direction
    uint64_t lb_resets;       // times the safeguard g.z > 0 cleared the memory
    // ---- QN_LS_STRONG_WOLFE (qn_vec_wolfe.hip.h): gtol, xtol, stpmin, the configured stpmax; then dcsrch's state between two trials ----
    double w_c2, w_xtol, w_tmin, w_tmax;
    double w_stpmax; // of this search: min(w_tmax, the box clip)
    double w_finit, w_ginit, w_gtest, w_width, w_width1, w_stx, w_fx, w_gx, w_sty, w_fy, w_gy, w_stmin, w_stmax;
    int32_t w_boxed, w_brackt, w_stage, w_err; // w_err: 1 = g.d >= 0 at the start, 2 = stpmax < stpmin
    int32_t tr_ls_cases, tr_ndigits;           // trace scratch: dcstep's cases of this iteration's search, base 8
    // ---- QN_NONLINEAR_CG (qn_cg.hip.h): the settings, then what survives calls like lambda ----
    int32_t cg_variant, cg_has_p; // QN_CG_*; cg_p holds the direction last searched (0: the next direction is -g, rule 1)
    double cg_powell_nu;          // Powell's restart test (+inf: off)
    int64_t cg_restart_every;     // 0: never
    double cg_beta;               // of the last accepted iteration: what the next direction is made with
    int64_t cg_since;             // iterations since the last -g direction
    uint64_t cg_restarts;         // betas that ended as exactly 0
    // ---- QN_LS_EXACT_QUADRATIC (qn_vec_exact.hip.h): the setting; what survives calls like lambda; this search's results; counters of this call ----
    int32_t ex_refresh_every;     // r: 1 every accepted point is evaluated by the objective, k > 1 every k-th, 0 never (but see ex_g_true)
    int32_t ex_g_true;            // g is the objective's own gradient at x, not the recurrence's: only then may the loop top declare convergence
    int64_t ex_since;             // accepted points since the objective last evaluated one
    int32_t ex_err, ex_adv;       // ex_err: 1 = g.d >= 0, 2 = curvature not positive and finite; ex_adv: this iteration's (f_t, gt) come from exact_advance_kernel
    double ex_c, ex_t;            // d'Qd and the step of the last search
    uint64_t ex_passes, ex_refreshes, ex_forced; // curvature passes; accepted points (and forced x) the objective evaluated; the forced ones among them
    // ---- QN_NEWTON_CG (qn_newton_cg.hip.h): the settings; the inner loop's scalars; counters of this call ----
    double tn_eta_max;                // the forcing term's cap, in (0, 1)
    int32_t tn_max_inner, tn_chunk;   // settings: inner steps at the most (0: min(n, 100)); inner steps enqueued per batch
    int32_t tn_cap, tn_state;         // max_inner resolved for this call; QN_TN_IDLE / QN_TN_RUNNING / QN_TN_ENDED
    int32_t tn_j, tn_exit;            // inner steps taken in this outer iteration; why the loop ended (QN_TN_EXIT_*)
    int32_t tn_zg, tn_use_g;          // rule 4 at j = 0: z = g; the direction is -g (rule 4 at j = 0, or rule 8's safeguard)
    double tn_gg, tn_sqgg, tn_rr, tn_eta, tn_kappa, tn_alpha, tn_beta, tn_gz;
    uint64_t tn_inner_last, tn_inner_total, tn_hv_passes, tn_neg_curv, tn_fallbacks;
    // ---- its preconditioner (qn_newton_cg.hip.h, rules 1' to 7'): the setting; r.(minv o r) beside tn_rr; counters of this call ----
    int32_t tn_precond, _pad3;        // QN_PRECOND_NONE / QN_PRECOND_JACOBI
    double tn_rz;
    uint64_t tn_diag_passes, tn_floored_last; // directions started with a diagonal; entries of the last minv that rule 2' set to 1
};
#define QN_TN_IDLE 0
#define QN_TN_RUNNING 1
#define QN_TN_ENDED 2
#define QN_TN_EXIT_TOL 1
#define QN_TN_EXIT_CAP 2
#define QN_TN_EXIT_NEGCURV 3

struct QnVecArgs {
    double *x, *g, *d, *xt, *gt;
    const double* z; // H^-1 g of the second-order variants (phase QN_VP_NSOLVE)
    const double *lb, *ub, *llb, *lub;
    double* part; // [QN_VEC_NPART][QN_VEC_MAXG]
    QnVecCtl* ctl;
    const double* f_dev;
    QnTraceRec* trace;
    double* xtrace;
    int n, np, G;
    // QN_LBFGS: the ring S[lb_m + 1][np], Y[lb_m + 1][np], the Gram kernel's shares, the small block (Gram matrices, u, gamma v), z for writing
    double *lS, *lY, *lpart, *lsmall, *zw;
    // QN_NONLINEAR_CG: the direction last searched (n_pad doubles, updated in place), the accept kernel's shares [QN_CG_NQ][QN_VEC_MAXG]
    double *cp, *cpart;
};

__device__ __forceinline__ double vec_block_max(double v, double* lds) { return ctl_block_fmax(v, lds); }
// QN_LS_STRONG_WOLFE's part of the loop top (qn_vec_wolfe.hip.h)
__device__ __forceinline__ double wolfe_min_parts(const double* part, int q, int G, double* lds);
__device__ __forceinline__ bool wolfe_start(QnVecCtl* c, double gd, double clip);
// QN_NONLINEAR_CG's part of the post kernel (qn_cg.hip.h): the eight sums (every thread), then beta by the rules (thread 0)
__device__ __forceinline__ void cg_post_sums(const QnVecArgs& a, double* q, double* lds);
__device__ __forceinline__ int cg_post(QnVecCtl* c, const double* q);

// d = P(x - lambda g) - x, three roundings per element in that order (spg.rs:81-83); PGD: x - g (projected_gradient_descent.rs:56-58).
// Before SPG has its lambda the same kernel forms P(x0 - g0) - x0, whose infinity norm gives lambda0 (spg.rs:41-46).
__global__ __launch_bounds__(QN_VEC_TPB) void vec_dir_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_EVAL_X && ph != QN_VP_DIR && ph != QN_VP_LS_ONLY && ph != QN_VP_NSOLVE) return;
    const bool scaled = vec_spectral(c->method) && c->has_lambda;
    const double lam = c->lambda;
    // projected_newton.rs:75-77, spn.rs:86-88: the step is z = H^-1 g, or lambda z.  (At their loop top -- QN_VP_EVAL_X / QN_VP_DIR -- this
    // kernel serves the projected gradient's norm, and P(x0 - g0) - x0 for lambda0, spn.rs:40-46.)
    const bool nsolve = ph == QN_VP_NSOLVE;
    double pg = 0.0, dm = 0.0, gd[1] = {0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d g = ld2(a.g + 2 * j);
        v2d d;
        if (ph == QN_VP_LS_ONLY) {
            d = ld2(a.d + 2 * j);
        } else {
            const v2d x = ld2(a.x + 2 * j), lo = ld2(a.lb + 2 * j), hi = ld2(a.ub + 2 * j);
            const v2d w = nsolve ? ld2(a.z + 2 * j) : g; // (the first-order family reads g once, as before)
            const double s0 = scaled ? lam * w.x : w.x, s1 = scaled ? lam * w.y : w.y;
            const double u0 = x.x - s0, u1 = x.y - s1;
            d.x = fmin(fmax(u0, lo.x), hi.x) - x.x;
            d.y = fmin(fmax(u1, lo.y), hi.y) - x.y;
            st2(a.d + 2 * j, d);
            // projected gradient with the exact comparisons of ls_solver.rs:124-129
            const double p0 = ((x.x == lo.x && g.x > 0.0) || (x.x == hi.x && g.x < 0.0)) ? 0.0 : g.x;
            const double p1 = ((x.y == lo.y && g.y > 0.0) || (x.y == hi.y && g.y < 0.0)) ? 0.0 : g.y;
            pg = fmax(pg, fmax(fabs(p0), fabs(p1)));
            dm = fmax(dm, fmax(fabs(d.x), fabs(d.y)));
        }
        gd[0] = gd[0] + g.x * d.x;
        gd[0] = gd[0] + g.y * d.y;
    }
    pg = vec_block_max(pg, lds);
    __syncthreads();
    dm = vec_block_max(dm, lds);
    __syncthreads();
    ctl_block_sum<1>(gd, lds);
    if (threadIdx.x == 0) {
        a.part[0 * QN_VEC_MAXG + blockIdx.x] = pg;
        a.part[1 * QN_VEC_MAXG + blockIdx.x] = gd[0];
        a.part[2 * QN_VEC_MAXG + blockIdx.x] = dm;
    }
}

// the G shares of quantity q, added (or maximised) in index order by one workgroup of QN_VEC_TPB threads
__device__ __forceinline__ double vec_sum_parts(const double* part, int q, int G, double* lds) {
    double v[1] = {0.0};
    for (int b = threadIdx.x; b < G; b += QN_VEC_TPB) v[0] = v[0] + part[q * QN_VEC_MAXG + b];
    __syncthreads();
    ctl_block_sum<1>(v, lds);
    return v[0];
}
__device__ __forceinline__ double vec_max_parts(const double* part, int q, int G, double* lds) {
    double v = 0.0;
    for (int b = threadIdx.x; b < G; b += QN_VEC_TPB) v = fmax(v, part[q * QN_VEC_MAXG + b]);
    __syncthreads();
    return vec_block_max(v, lds);
}

// the line search has returned ctl->t: decide what the update step needs (thread 0)
__device__ __forceinline__ void vec_ls_return(QnVecCtl* c, bool evaluated) {
    c->ls_result = c->t;
    if (c->ls_only) { c->status = QN_OK; c->phase = QN_VP_DONE; return; }
    c->gt_valid = evaluated ? 1 : 0;
    if (vec_needs_y(c->method)) {
        if (evaluated && c->memoize) { c->n_calls++; c->tr_n_evals++; c->phase = QN_VP_ACCEPT; } // spg.rs:130 at the point the search accepted
        else { c->gt_valid = 0; c->phase = QN_VP_REEVAL; }
    } else {
        if (!c->memoize) c->gt_valid = 0; // the loop top evaluates x_next itself
        c->phase = QN_VP_ACCEPT;
    }
}

// the loop top of ls_solver.rs:79-90 behind the oracle call (thread 0): true when the run ends here
__device__ __forceinline__ bool vec_loop_top(QnVecCtl* c, double pg) {
    c->tr_n_evals++;
    if (isnan(c->f_cur) || isinf(c->f_cur)) { c->status = QN_OUT_OF_DOMAIN; c->phase = QN_VP_DONE; return true; } // ls_solver.rs:37-40
    c->pgnorm = pg;
    if (c->method == QN_PROJECTED_NEWTON && c->has_sy) { // projected_newton.rs:98-103: s_norm, then y_norm, then the projected gradient
        if (c->s_norm < c->tol) { c->status = QN_OK; c->phase = QN_VP_DONE; return true; }
        if (c->y_norm < c->tol) { c->status = QN_OK; c->phase = QN_VP_DONE; return true; }
    }
    if (pg < c->tol && c->ls_kind == QN_LS_EXACT_QUADRATIC && !c->ex_g_true) { // the test passed on a recurrence gradient: the objective evaluates x, then the loop top again
        c->have_eval = 0; c->ex_refreshes++; c->ex_forced++; c->phase = QN_VP_EXACT_REFRESH;
        return true;
    }
    if (pg < c->tol) { c->status = QN_OK; c->phase = QN_VP_DONE; return true; } // spg.rs:89-92
    c->tr_f = c->f_cur; c->tr_gnorm = pg;
    return false;
}

__global__ __launch_bounds__(QN_VEC_TPB) void vec_top_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_EVAL_X && ph != QN_VP_DIR && ph != QN_VP_LS_ONLY && ph != QN_VP_NSOLVE) return;
    const double pg = vec_max_parts(a.part, 0, a.G, lds);
    const double gd = vec_sum_parts(a.part, 1, a.G, lds);
    const double dm = vec_max_parts(a.part, 2, a.G, lds);
    double clip = INFINITY; // StrongWolfe's boxed form: the largest step that stays inside the search's box (wolfe_clip_kernel's shares)
    if (c->ls_kind == QN_LS_STRONG_WOLFE && c->w_boxed && ph != QN_VP_LS_ONLY) clip = wolfe_min_parts(a.part, 6, a.G, lds);
    if (threadIdx.x != 0) return;
    if (ph == QN_VP_EVAL_X) { c->f_cur = *a.f_dev; c->have_eval = 1; c->n_evals++; c->ex_g_true = 1; c->ex_since = 0; } // (ex_*: QN_LS_EXACT_QUADRATIC's, read by no other kind)
    if (ph != QN_VP_LS_ONLY && ph != QN_VP_NSOLVE) {
        c->n_calls++;
        if (vec_spectral(c->method) && !c->has_lambda) { // spg.rs:40-46: the constructor's call; d was formed with lambda = 1
            c->lambda = fmax(fmin(1.0 / dm, c->lambda_max), c->lambda_min);
            c->has_lambda = 1;
            if (c->max_iter <= 0) { c->status = QN_MAX_ITER_REACHED; c->phase = QN_VP_DONE; return; }
            c->phase = c->memoize ? QN_VP_DIR : QN_VP_EVAL_X;
            return;
        }
        if (vec_loop_top(c, pg)) return;
        if (vec_nsolve(c->method)) { c->phase = QN_VP_NSOLVE; return; } // the direction needs the factorisation (QN_LBFGS: the two streams of its memory): enqueued for this phase only
    }
    c->gd = gd;
    if (c->ls_kind == QN_LS_EXACT_QUADRATIC) { // no first trial of 1: the curvature pass and exact_step_kernel make the step (qn_vec_exact.hip.h)
        c->ls_i = 0;
        if (!(gd < 0.0)) { c->ex_err = 1; c->status = QN_ABNORMAL_TERMINATION; c->phase = QN_VP_DONE; return; }
        c->phase = QN_VP_EXACT;
        return;
    }
    if (c->ls_kind == QN_LS_GLL_QUADRATIC) { // gll_quadratic.rs:62-64: append_new_f, then f_max once
        if (c->ring_len == c->m) {
            for (int i = 1; i < c->ring_len; ++i) c->ring[i - 1] = c->ring[i];
            c->ring_len--;
        }
        c->ring[c->ring_len++] = c->f_cur;
        double fm = -INFINITY;
        for (int i = 0; i < c->ring_len; ++i) fm = fmax(c->ring[i], fm);
        c->f_max = fm;
    }
    c->t = 1.0;
    c->ls_i = 0;
    if (c->ls_kind == QN_LS_STRONG_WOLFE && !wolfe_start(c, gd, clip)) return; // dcsrch's START: stpmax of this search, the first trial into c->t
    if (c->max_iter_ls <= 0) vec_ls_return(c, false);
    else c->phase = QN_VP_TRIAL;
}

__global__ __launch_bounds__(QN_VEC_TPB) void vec_trial_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) return;
    const bool project = ph == QN_VP_TRIAL && c->ls_kind == QN_LS_BACKTRACKING_B; // backtracking_b.rs:65-67
    const double t = c->t;
    double diff2[1] = {0.0}, moved = 0.0;
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), d = ld2(a.d + 2 * j);
        const double td0 = t * d.x, td1 = t * d.y; // `t * direction_k` rounds first
        v2d u;
        u.x = x.x + td0;
        u.y = x.y + td1;
        if (project) {
            const v2d lo = ld2(a.llb + 2 * j), hi = ld2(a.lub + 2 * j);
            v2d p;
            p.x = fmin(fmax(u.x, lo.x), hi.x);
            p.y = fmin(fmax(u.y, lo.y), hi.y);
            if (p.x != u.x || p.y != u.y) moved = 1.0;
            const double e0 = p.x - x.x, e1 = p.y - x.y;
            diff2[0] = diff2[0] + e0 * e0;
            diff2[0] = diff2[0] + e1 * e1;
            u = p;
        }
        st2(a.xt + 2 * j, u);
    }
    if (!project) return;
    moved = vec_block_max(moved, lds);
    __syncthreads();
    ctl_block_sum<1>(diff2, lds);
    if (threadIdx.x == 0) {
        a.part[0 * QN_VEC_MAXG + blockIdx.x] = diff2[0];
        a.part[1 * QN_VEC_MAXG + blockIdx.x] = moved;
    }
}

__global__ __launch_bounds__(QN_VEC_TPB) void vec_decide_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    QnVecCtl* c = a.ctl;
    const int ph = c->phase;
    if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) return;
    double diff2 = 0.0, moved = 0.0;
    if (ph == QN_VP_TRIAL && c->ls_kind == QN_LS_BACKTRACKING_B) {
        diff2 = vec_sum_parts(a.part, 0, a.G, lds);
        moved = vec_max_parts(a.part, 1, a.G, lds);
    }
    if (threadIdx.x != 0) return;
    const double ft = *a.f_dev;
    c->f_t = ft;
    c->n_calls++; c->n_evals++; c->tr_n_evals++;
    if (ph == QN_VP_REEVAL) { c->gt_valid = 1; c->phase = QN_VP_ACCEPT; return; }
    c->tr_ls_iters++;
    const double t = c->t, gd = c->gd, fk = c->f_cur;
    if (c->ls_kind == QN_LS_GLL_QUADRATIC) {
        if (ft - c->f_max <= c->c1 * t * gd) { vec_ls_return(c, true); return; } // gll_quadratic.rs:73, mod.rs:35
        if (t <= 0.1) {
            c->t = t * 0.5; // :78-80
        } else {
            const double t_tmp = -0.5 * t * t * gd / (ft - fk - t * gd); // :83-84
            if (t_tmp > c->sigma1 && t_tmp < c->sigma2 * t) c->t = t_tmp; // :85-87
            else c->t = t_tmp * 0.5;                                       // :91
        }
        c->ls_i++;
    } else {
        if (isnan(ft) || isinf(ft)) { // backtracking.rs:37-41, backtracking_b.rs:70-74: `continue` without i += 1
            c->t = t * c->beta;
            return;
        }
        const bool ok = c->ls_kind == QN_LS_BACKTRACKING_B ? (ft - fk <= (-c->c1 / t) * diff2) // backtracking_b.rs:32-33
                                                           : (ft - fk <= c->c1 * t * gd);      // mod.rs:35
        if (ok) { vec_ls_return(c, moved == 0.0); return; } // (a projected trial that moved is not x + t d: next_iterate is, projected_gradient_descent.rs:103)
        c->t = t * c->beta;
        c->ls_i++;
    }
    if (c->ls_i >= c->max_iter_ls) vec_ls_return(c, false); // "Max iter reached. Early stopping.": t was never evaluated
}

// x_next = x + t d (spg.rs:126), s = x_next - x, y = g(x_next) - g(x) (:129-130); x <- x_next, g <- g(x_next) where it is known
__global__ __launch_bounds__(QN_VEC_TPB) void vec_accept_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_ACCEPT) return;
    const bool have_gt = c->gt_valid != 0;
    const double t = c->t;
    const int64_t row = (int64_t)c->n_iter;
    const bool xtr = c->trace_x && a.xtrace && row < c->trace_cap;
    double acc[2] = {0.0, 0.0};
    const bool second = vec_newton(c->method) && have_gt; // also y.y, and the projected gradient at (x_next, g(x_next)) for the next loop top
    double yy[1] = {0.0}, pgn = 0.0;
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), d = ld2(a.d + 2 * j);
        const double td0 = t * d.x, td1 = t * d.y;
        v2d xn;
        xn.x = x.x + td0;
        xn.y = x.y + td1;
        const double s0 = xn.x - x.x, s1 = xn.y - x.y;
        acc[1] = acc[1] + s0 * s0;
        acc[1] = acc[1] + s1 * s1;
        if (have_gt) {
            const v2d g = ld2(a.g + 2 * j), gt = ld2(a.gt + 2 * j);
            const double y0 = gt.x - g.x, y1 = gt.y - g.y;
            acc[0] = acc[0] + s0 * y0;
            acc[0] = acc[0] + s1 * y1;
            st2(a.g + 2 * j, gt);
            if (second) {
                yy[0] = yy[0] + y0 * y0;
                yy[0] = yy[0] + y1 * y1;
                const v2d lo = ld2(a.lb + 2 * j), hi = ld2(a.ub + 2 * j);
                const double p0 = ((xn.x == lo.x && gt.x > 0.0) || (xn.x == hi.x && gt.x < 0.0)) ? 0.0 : gt.x;
                const double p1 = ((xn.y == lo.y && gt.y > 0.0) || (xn.y == hi.y && gt.y < 0.0)) ? 0.0 : gt.y;
                pgn = fmax(pgn, fmax(fabs(p0), fabs(p1)));
            }
        }
        st2(a.x + 2 * j, xn);
        if (xtr) {
            if (2 * j < a.n) a.xtrace[(size_t)row * a.n + 2 * j] = xn.x;
            if (2 * j + 1 < a.n) a.xtrace[(size_t)row * a.n + 2 * j + 1] = xn.y;
        }
    }
    ctl_block_sum<2>(acc, lds);
    if (threadIdx.x == 0) {
        a.part[2 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        a.part[3 * QN_VEC_MAXG + blockIdx.x] = acc[1];
    }
    if (!second) return;
    pgn = vec_block_max(pgn, lds);
    ctl_block_sum<1>(yy, lds);
    if (threadIdx.x == 0) {
        a.part[4 * QN_VEC_MAXG + blockIdx.x] = pgn;
        a.part[5 * QN_VEC_MAXG + blockIdx.x] = yy[0];
    }
}

__global__ __launch_bounds__(QN_VEC_TPB) void vec_post_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_ACCEPT) return;
    const double sy = vec_sum_parts(a.part, 2, a.G, lds);
    const double ss = vec_sum_parts(a.part, 3, a.G, lds);
    const bool second = vec_newton(c->method) && c->gt_valid;
    const bool lbfgs = c->method == QN_LBFGS || c->method == QN_OWLQN; // (lbfgs_accept_kernel, or owl_accept_kernel, ran in vec_accept_kernel's place)
    double pgn = 0.0, yy = 0.0;
    if (second) {
        pgn = vec_max_parts(a.part, 4, a.G, lds);
        yy = vec_sum_parts(a.part, 5, a.G, lds);
    }
    if (lbfgs) yy = vec_sum_parts(a.part, 5, a.G, lds);
    const bool cg = c->method == QN_NONLINEAR_CG; // (cg_accept_kernel ran in vec_accept_kernel's place)
    double cq[8];
    if (cg) cg_post_sums(a, cq, lds);
    if (threadIdx.x != 0) return;
    int committed = 0;
    if (cg) committed = cg_post(c, cq); // beta for the next direction; `updated` = beta != 0
    if (lbfgs && sy > DBL_EPSILON * yy) { // the pair in the staging slot joins the memory; otherwise the memory stays as it was
        committed = 1;
        if (c->lb_kmem == c->lb_m) c->lb_head = (c->lb_head + 1) % (c->lb_m + 1); // (the oldest pair's slot is the next staging slot)
        else c->lb_kmem++;
    }
    if (c->method == QN_PROJECTED_NEWTON) { c->s_norm = sqrt(ss); c->y_norm = sqrt(yy); c->has_sy = 1; } // projected_newton.rs:132-135
    if (vec_spectral(c->method)) { // spg.rs:135-143, spn.rs:140-147
        if (sy <= 0.0) c->lambda = c->lambda_max;
        else c->lambda = fmax(fmin(ss / sy, c->lambda_max), c->lambda_min);
    }
    if (a.trace && (int64_t)c->n_iter < c->trace_cap) {
        QnTraceRec r;
        r.f = c->tr_f; r.gnorm = c->tr_gnorm; r.t = c->t; r.s_norm = (vec_spectral(c->method) || c->method == QN_PROJECTED_NEWTON || lbfgs || cg) ? sqrt(ss) : 0.0;
        r.y_norm = c->method == QN_PROJECTED_NEWTON ? sqrt(yy) : 0.0;
        r.n_evals = c->tr_n_evals; r.ls_iters = c->tr_ls_iters; r.ls_cases = c->tr_ls_cases; r.updated = committed;
        a.trace[c->n_iter] = r;
    }
    c->have_eval = c->gt_valid;
    if (c->gt_valid) c->f_cur = c->f_t;
    c->tr_n_evals = 0; c->tr_ls_iters = 0; c->tr_ls_cases = 0; c->tr_ndigits = 0;
    c->k++; c->n_iter++; // ls_solver.rs:104
    if (c->k >= c->max_iter) { c->status = QN_MAX_ITER_REACHED; c->phase = QN_VP_DONE; return; } // :78, :110
    c->phase = (c->have_eval && c->memoize) ? QN_VP_DIR : QN_VP_EVAL_X;
    // The second-order variants on a memoised oracle: (f, g) at x_next are the accepted evaluation, so the next loop top (its oracle call is
    // the memo's) is decided HERE, from the accept kernel's projected-gradient norm.  The host's one peek per batch then knows whether a
    // factorisation is wanted at all: a converged or capped run enqueues none.
    if (second && c->phase == QN_VP_DIR) {
        c->n_calls++;
        if (vec_loop_top(c, pgn)) return;
        c->phase = QN_VP_NSOLVE;
    }
}

// ---- n <= QN_SMALL_N: z = H^-1 g as nalgebra's `cholesky().unwrap().solve(g)` computes it, operation for operation, one thread ----
// Cholesky::new (column by column: col_j -= L[j][k] col_k as an axpy of two roundings, sqrt of the diagonal, the column divided by it), then
// solve_lower_triangular (column-oriented: b[i] /= L[i][i]; b[i+1..] -= b[i] L[i+1..][i]) and ad_solve_lower_triangular (row-oriented:
// b[i] = (b[i] - L[i+1..][i] . b[i+1..]) / L[i][i]).  Only the lower triangle of H is read.  z is zero-padded to n_pad.
__global__ void pn_small_kernel(const double* __restrict__ Hrow, size_t ld, int n, int n_pad, const double* __restrict__ g, double* __restrict__ z,
                                int* __restrict__ fail) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a[QN_SMALL_N * QN_SMALL_N], b[QN_SMALL_N]; // column-major
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) a[i + j * n] = Hrow[(size_t)i * ld + j];
    for (int j = 0; j < n; ++j) {
        for (int k = 0; k < j; ++k) {
            const double factor = -a[j + k * n];
            for (int i = j; i < n; ++i) { const double pr = factor * a[i + k * n]; a[i + j * n] = pr + a[i + j * n]; }
        }
        const double diag = a[j + j * n];
        if (!(diag > 0.0)) { *fail = 1; return; } // (zero, negative or NaN: Cholesky::new returns None and the reference's unwrap panics)
        const double denom = sqrt(diag);
        a[j + j * n] = denom;
        for (int i = j + 1; i < n; ++i) a[i + j * n] = a[i + j * n] / denom;
    }
    for (int i = 0; i < n; ++i) b[i] = g[i];
    for (int i = 0; i < n; ++i) {
        const double coeff = b[i] / a[i + i * n];
        b[i] = coeff;
        for (int r = i + 1; r < n; ++r) { const double pr = -coeff * a[r + i * n]; b[r] = pr + b[r]; }
    }
    for (int i = n - 1; i >= 0; --i) {
        double dot = 0.0;
        for (int r = i + 1; r < n; ++r) { const double pr = a[r + i * n] * b[r]; dot = dot + pr; }
        b[i] = (b[i] - dot) / a[i + i * n];
    }
    for (int i = 0; i < n_pad; ++i) z[i] = i < n ? b[i] : 0.0;
}
