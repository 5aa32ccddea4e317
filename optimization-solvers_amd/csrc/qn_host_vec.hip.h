// qn_host_vec.hip.h -- host side of the first-order family (QN_SPG, QN_PROJECTED_GRADIENT; kernels: qn_vec.hip.h): GLLQuadratic's and StrongWolfe's
// builders, the SPG setters, and the pump.  The pump takes no decision: it enqueues one iteration's kernels -- every one predicated on QnVecCtl.phase --
// and reads the control block back with one small copy per batch (a 700-byte hipMemcpyAsync into pinned memory in front of the one
// synchronisation the batch needs anyway: no second mapping to keep coherent, no fence in the one-workgroup kernels).
#pragma once

extern "C" void qn_gll_quadratic_new(qn_linesearch* ls, double c1, size_t m) { // GLLQuadratic::new, gll_quadratic.rs:13-23
    memset(ls, 0, sizeof(*ls));
    ls->kind = QN_LS_GLL_QUADRATIC;
    ls->c1 = c1;
    ls->_pad = m > (size_t)INT32_MAX ? INT32_MAX : (int32_t)m;
    ls->delta_min = 0.1; ls->delta_max = 0.9; // sigma1, sigma2
}
extern "C" void qn_gll_quadratic_with_sigmas(qn_linesearch* ls, double sigma1, double sigma2) { // :24-28
    ls->delta_min = sigma1; ls->delta_max = sigma2;
}

// StrongWolfe (QN_LS_STRONG_WOLFE, kernels: qn_vec_wolfe.hip.h): MINPACK-2 dcsrch; ftol = c1, gtol = c2, xtol in `delta`, stpmin = t_min, stpmax = t_max
extern "C" void qn_strong_wolfe_new(qn_linesearch* ls, double c1, double c2) {
    memset(ls, 0, sizeof(*ls));
    ls->kind = QN_LS_STRONG_WOLFE;
    ls->c1 = c1; ls->c2 = c2; // (0 < c1 < c2 < 1 is checked by qn_minimize: this constructor returns nothing)
    ls->delta = 0.1; ls->t_min = 0.0; ls->t_max = 1e10;
}
extern "C" int qn_strong_wolfe_with_xtol(qn_linesearch* ls, double xtol) {
    if (!ls || ls->kind != QN_LS_STRONG_WOLFE) return fail(QN_ERROR_INPUT_PARAMS, "xtol belongs to a StrongWolfe line search");
    if (!(xtol >= 0.0)) return fail(QN_ERROR_INPUT_PARAMS, "StrongWolfe: xtol must not be negative");
    ls->delta = xtol;
    return QN_OK;
}

static bool pn_method(int method) { return method == QN_PROJECTED_NEWTON || method == QN_SPECTRAL_PROJECTED_NEWTON; }
static bool spectral_method(int method) { return method == QN_SPG || method == QN_SPECTRAL_PROJECTED_NEWTON || method == QN_SPECTRAL_PROXIMAL_GRADIENT; }
static bool vec_method(int method) { return method == QN_SPG || method == QN_PROJECTED_GRADIENT || pn_method(method) || method == QN_LBFGS || method == QN_NONLINEAR_CG || method == QN_NEWTON_CG || method == QN_SPECTRAL_PROXIMAL_GRADIENT || method == QN_OWLQN; }
struct VecRun;
static int lbfgs_state_alloc(qn_solver* s); // QN_LBFGS: qn_host_lbfgs.hip.h
static int lbfgs_enqueue_direction(VecRun& r, bool wolfe_clip);
static int lbfgs_enqueue_accept(VecRun& r);
static int cg_state_alloc(qn_solver* s); // QN_NONLINEAR_CG: qn_host_cg.hip.h
static int cg_enqueue_direction(VecRun& r);
static int cg_enqueue_accept(VecRun& r);
static int exact_state_alloc(qn_solver* s); // QN_LS_EXACT_QUADRATIC: qn_vec_exact.hip.h
static int tn_state_alloc(qn_solver* s); // QN_NEWTON_CG: qn_host_newton_cg.hip.h
static int tn_check(const qn_solver* s, const qn_linesearch* ls, const qn_objective* obj, int ls_only);
static int tn_enqueue_direction(VecRun& r, bool fresh, uint64_t* weights_passes);
static int tn_precond_alloc(qn_solver* s);
static int exact_enqueue_step(VecRun& r);
static int exact_enqueue_advance(VecRun& r);
static int prox_state_alloc(qn_solver* s); // QN_SPECTRAL_PROXIMAL_GRADIENT: qn_host_prox.hip.h
static int prox_check(const qn_solver* s, const qn_linesearch* ls, int ls_only);
static int prox_enqueue_direction(VecRun& r);
static int prox_enqueue_trial(VecRun& r);
static int prox_enqueue_decide(VecRun& r);
static int owl_state_alloc(qn_solver* s); // QN_OWLQN: qn_host_owlqn.hip.h
static int owl_check(const qn_solver* s, const qn_linesearch* ls, int ls_only);
static int owl_enqueue_direction(VecRun& r);
static int owl_enqueue_trial(VecRun& r);
static int owl_enqueue_decide(VecRun& r);
static int owl_enqueue_accept(VecRun& r);
static int vec_grid(size_t np) { // a function of n alone: four 16-byte accesses per thread until 4 workgroups per CU are out
    const size_t per = (size_t)QN_VEC_TPB * 2 * 4;
    return (int)std::min<size_t>(QN_VEC_MAXG, std::max<size_t>(1, (np + per - 1) / per));
}

// O(n) only: the control block and the partials; the vectors are the solver's work vectors (no H, no n x n scratch)
static int vec_state_alloc(qn_solver* s) {
    if (s->vctl) return QN_OK;
    hipStream_t st = s->ctx->stream;
    QNCHK(s->vctl.alloc_zero(1, st));
    QNCHK(s->hvctl.alloc_zero(1));
    s->hvctl->lambda_min = 1e-3; s->hvctl->lambda_max = 1e3; // spg.rs:36-37
    QNCHK(s->vpart.alloc_zero((size_t)QN_VEC_NPART * QN_VEC_MAXG, st));
    QNCHK(bounds_alloc(s)); // the box is (-inf, +inf) until qn_solver_set_bounds
    if (s->method == QN_LBFGS) QNCHK(lbfgs_state_alloc(s));
    if (s->method == QN_NONLINEAR_CG) QNCHK(cg_state_alloc(s));
    if (s->method == QN_NEWTON_CG) QNCHK(tn_state_alloc(s));
    if (s->method == QN_SPECTRAL_PROXIMAL_GRADIENT) QNCHK(prox_state_alloc(s));
    if (s->method == QN_OWLQN) QNCHK(owl_state_alloc(s));
    return QN_OK;
}
static void vec_state_reset(qn_solver* s) { // back to the state right after ::new: no lambda, an empty f_previous, no memo
    if (!s->hvctl) return;
    QnVecCtl* h = s->hvctl;
    h->has_lambda = 0; h->lambda = 0.0; h->have_eval = 0; h->ring_len = 0; h->k = 0; h->n_iter = 0;
    h->lb_kmem = 0; h->lb_head = 0; h->lb_gamma = 1.0; h->lb_resets = 0; // QN_LBFGS: an empty memory (lb_m and the scaling switch are settings: kept)
    h->cg_has_p = 0; h->cg_beta = 0.0; h->cg_since = 0; h->cg_restarts = 0; // QN_NONLINEAR_CG: no direction yet (the variant, nu and restart_every are settings: kept)
    h->tn_state = 0; h->tn_inner_last = 0; h->tn_inner_total = 0; h->tn_hv_passes = 0; h->tn_neg_curv = 0; h->tn_fallbacks = 0; // QN_NEWTON_CG: no inner loop has run (eta_max, max_inner, chunk and the preconditioner are settings: kept)
    h->tn_diag_passes = 0; h->tn_floored_last = 0;
    h->ex_since = 0; h->ex_g_true = 0; // QN_LS_EXACT_QUADRATIC: no accepted point yet (the next evaluation at x is the objective's: have_eval is 0)
    h->has_sy = 0; h->s_norm = 0.0; h->y_norm = 0.0; // (the Cholesky factor of a device quadratic's Hessian is kept: it is keyed on the objective)
}

extern "C" int qn_solver_set_spg_lambdas(qn_solver* s, double lambda_min, double lambda_max) { // with_lambdas, spg.rs:23-27
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (!spectral_method(s->method)) return fail(QN_ERROR_INPUT_PARAMS, "lambda bounds belong to a SpectralProjectedGradient / SpectralProjectedNewton solver");
    s->hvctl->lambda_min = lambda_min; s->hvctl->lambda_max = lambda_max; // (the current lambda is not clamped again, as in the reference)
    return QN_OK;
}
extern "C" int qn_solver_newton_factorisations(qn_solver* s, size_t* out) {
    if (!s || !out) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    *out = (size_t)s->pn_factorisations;
    return QN_OK;
}
extern "C" int qn_solver_spg_lambda(qn_solver* s, double* out, int* is_some) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (!spectral_method(s->method)) return fail(QN_ERROR_INPUT_PARAMS, "lambda belongs to a SpectralProjectedGradient / SpectralProjectedNewton solver");
    if (is_some) *is_some = s->hvctl->has_lambda;
    if (out) *out = s->hvctl->lambda;
    return QN_OK;
}

// The two vectors an audit of a run needs exactly (tests/newton_cg_audit.py): n doubles copied from the solver's own vectors on its stream.  No
// launch, and nothing a run reads is written: a run that never calls them is the run it was.  INSIDE THE CALLBACK the pump has synchronised
// (vec_peek) and enqueued nothing behind the batch that accepted iteration k: V.d is still d_k -- the next batch's vec_dir_kernel is what
// overwrites it -- and V.g is g(x_{k+1}) where the accept kernel stored the accepted trial's gradient (a memoised oracle: have_eval).
extern "C" int qn_solver_get_direction(qn_solver* s, double* d_host) {
    if (!s || !d_host) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (!vec_method(s->method)) return fail(QN_ERROR_INPUT_PARAMS, "get_direction: built for the vector family (SPG, projected gradient, projected Newton, L-BFGS, NonlinearCG, NewtonCG)");
    if (!s->vec_d_searched)
        return fail(QN_ERROR_INPUT_PARAMS, "get_direction: no searched direction is held (no iteration has been accepted, or the last loop top ended the run and left P(x - g) - x in its place)");
    HIPCHK(hipSetDevice(s->ctx->device));
    HIPCHK(hipMemcpyAsync(d_host, s->V.d, s->n * sizeof(double), hipMemcpyDeviceToHost, s->ctx->stream));
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    return QN_OK;
}
extern "C" int qn_solver_get_gradient(qn_solver* s, double* g_host) {
    if (!s || !g_host) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (!vec_method(s->method)) return fail(QN_ERROR_INPUT_PARAMS, "get_gradient: built for the vector family (SPG, projected gradient, projected Newton, L-BFGS, NonlinearCG, NewtonCG)");
    if (!s->hvctl || !s->hvctl->have_eval || !s->hctl->have_cur_eval)
        return fail(QN_ERROR_INPUT_PARAMS, "get_gradient: no evaluation at the current x is held (nothing has been evaluated yet -- an iteration cap of 0 evaluates nothing --, the oracle is not memoised, or x was set since)");
    HIPCHK(hipSetDevice(s->ctx->device));
    HIPCHK(hipMemcpyAsync(g_host, s->V.g, s->n * sizeof(double), hipMemcpyDeviceToHost, s->ctx->stream));
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    return QN_OK;
}

// ComputeDirection::compute_direction on its own: P(x - lambda g) - x (spg.rs:76-86), P(x - g) - x (projected_gradient_descent.rs:51-60)
static int vec_compute_direction(qn_solver* s, const double* g_host, double* d_host) {
    const size_t n = s->n, np = s->T.n_pad;
    if (pn_method(s->method)) return fail(QN_ERROR_INPUT_PARAMS, "the projected Newton direction needs the oracle's Hessian: use qn_minimize");
    if (s->method == QN_LBFGS) return fail(QN_ERROR_INPUT_PARAMS, "the L-BFGS direction is formed from the device-resident memory: use qn_minimize");
    if (s->method == QN_NONLINEAR_CG) return fail(QN_ERROR_INPUT_PARAMS, "the NonlinearCG direction is formed from the device-resident previous direction: use qn_minimize");
    if (s->method == QN_NEWTON_CG) return fail(QN_ERROR_INPUT_PARAMS, "the NewtonCG direction is formed by an inner loop on the device objective: use qn_minimize");
    if (s->method == QN_SPECTRAL_PROXIMAL_GRADIENT) return fail(QN_ERROR_INPUT_PARAMS, "the SpectralProximalGradient direction is formed by the device's proximal map: use qn_minimize");
    if (s->method == QN_OWLQN) return fail(QN_ERROR_INPUT_PARAMS, "the OWLQN direction is formed from the device-resident memory and pseudo-gradient: use qn_minimize");
    if (s->method == QN_SPG && !s->hvctl->has_lambda) return fail(QN_ERROR_INPUT_PARAMS, "lambda0 needs the oracle: the first qn_minimize evaluates it");
    std::vector<double> x(n), lb(n), ub(n);
    QNCHK(qn_solver_get_x(s, x.data()));
    HIPCHK(hipMemcpy(lb.data(), s->bounds_block, n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ub.data(), s->bounds_block + np, n * sizeof(double), hipMemcpyDeviceToHost));
    const double lam = s->hvctl->lambda;
    for (size_t i = 0; i < n; ++i) {
        const double step = s->method == QN_SPG ? lam * g_host[i] : g_host[i];
        const double u = x[i] - step;
        d_host[i] = std::fmin(std::fmax(u, lb[i]), ub[i]) - x[i];
    }
    return QN_OK;
}

struct VecRun {
    qn_solver* s;
    const qn_oracle* o;
    qn_objective* obj;
    QnVecArgs a;
};

static int vec_peek(VecRun& r, bool with_xt) { // the one small copy, and the batch's synchronisation
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    if (with_xt) HIPCHK(hipMemcpyAsync(s->hx, s->V.xt, s->n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s->hvctl, s->vctl, sizeof(QnVecCtl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->stats.host_syncs++;
    return QN_OK;
}

// the oracle at V.xt -> (f_dev, V.gt); unconditional (a closure cannot be predicated): the kernels behind it are
static int vec_enqueue_eval(VecRun& r) {
    qn_solver* s = r.s;
    qn_context* c = s->ctx;
    hipStream_t st = c->stream;
    if (r.obj) { // a device objective: its table's launches.  d or P goes to the kind's trial buffer (the weights at x_k stay NewtonCG's)
        const QnObjOps* ops = r.obj->ops;
        const QnObjWork w{s->V.q, s->V.s}; // the dense quadratic's (row-block 0 stores its copy of the point: V.s is free here)
        if (ops->eval_split) { // the streaming launches, then the finish: profiling mode times the two apart, t_eval_ms is the stream alone
            { ProfScope ps(s, KC_EVAL); QNCHK(ops->eval(r.obj, s->V.xt, s->f_dev, s->V.gt, 1, &w)); }
            { ProfScope ps(s, KC_CTL); QNCHK(ops->eval(r.obj, s->V.xt, s->f_dev, s->V.gt, 2, &w)); }
        } else {
            ProfScope ps(s, KC_EVAL);
            QNCHK(ops->eval(r.obj, s->V.xt, s->f_dev, s->V.gt, 3, &w));
        }
        if (ops->vec_counted) s->stats.launches += ops->eval_launches;
        return QN_OK;
    }
    ProfScope ps(s, KC_EVAL);
    if (r.o->kind == QN_ORACLE_HOST) { // s->hx holds xt (vec_peek)
        double f = NAN;
        if (r.o->host_fn(r.o->host_user, s->hx, s->n, &f, s->hg) != 0) return fail(QN_ABNORMAL_TERMINATION, "host oracle returned non-zero");
        s->hg[s->n] = f;
        HIPCHK(hipMemcpyAsync(s->V.gt, s->hg, s->n * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->f_dev, s->hg + s->n, sizeof(double), hipMemcpyHostToDevice, st));
        return QN_OK;
    }
    if (r.o->kind == QN_ORACLE_DEVICE_FN) {
        if (r.o->device_fn(r.o->device_user, (void*)st, s->V.xt, s->n, s->f_dev, s->V.gt) != 0)
            return fail(QN_ABNORMAL_TERMINATION, "device oracle returned non-zero");
        return QN_OK;
    }
    return fail(QN_ERROR_INPUT_PARAMS, "unknown oracle kind");
}

// ProjectedNewton / SpectralProjectedNewton, phase QN_VP_NSOLVE: z = H^-1 g into V.y -- `hessian.cholesky().unwrap().solve(eval.g())`
// (projected_newton.rs:75, spn.rs:86): ONE factorisation (newton_chol_factor, the lower triangle only) and ONE solve.  The Hessian of a device
// quadratic is the same matrix in every iteration: its factor in newton_w (and the block inverses) is kept, keyed on the objective's serial,
// and later iterations run the solve alone -- the same bits as factorising again (QN_OPT_PNEWTON_REUSE_FACTOR 0 does that).  A host closure's
// Hessian is asked for, and factorised, in every iteration that computes a direction.  No LU fallback: the reference unwraps.
static int pn_enqueue_solve(VecRun& r) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    ProfScope ps(s, KC_NEWTON);
    const int n = (int)s->n, n64 = (int)s->newton_n64;
    const uint64_t serial = r.obj ? r.obj->serial : 0;
    const bool small = s->n <= QN_SMALL_N;
    const bool reuse = !small && s->pn_reuse && serial != 0 && s->pn_factor_serial == serial;
    if (!reuse) {
        const double* hsrc = nullptr;
        size_t ld_src = 0;
        bool symmetric = true; // (not consulted: only the lower triangle is read, as nalgebra's Cholesky does)
        s->pn_factor_serial = 0;
        QNCHK(newton_stage_hessian(s, r.o, r.obj, &hsrc, &ld_src, &symmetric));
        HIPCHK(hipMemsetAsync(s->newton_fail, 0, 2 * sizeof(int), st));
        s->pn_factorisations++;
        if (small) {
            hipLaunchKernelGGL(pn_small_kernel, dim3(1), dim3(64), 0, st, hsrc, ld_src, n, (int)s->T.n_pad, s->V.g, s->V.y, s->newton_fail);
            s->stats.launches++;
        } else {
            QNCHK(newton_chol_factor(s, hsrc, ld_src));
        }
    }
    if (!small) {
        double* x1 = s->newton_x;
        double* x2 = s->newton_x + n64;
        const dim3 vg(std::min(1024, (n64 + 255) / 256)), vb(256);
        hipLaunchKernelGGL(newton_vec_kernel, vg, vb, 0, st, x1, s->V.g, n, n64, 1.0);
        QNCHK(newton_tri_solve(s, x1, x2));
        hipLaunchKernelGGL(newton_vec_kernel, vg, vb, 0, st, s->V.y, x1, n, s->T.n_pad, 1.0);
        s->stats.launches += 2 + (s->newton_big ? 0 : 2 * (uint64_t)(n64 / QN_NB));
    }
    HIPCHK(hipGetLastError());
    if (reuse) return QN_OK; // (the kept factor was checked when it was made)
    int chol_failed = 0; // read here, behind everything enqueued, as Newton's direction does
    HIPCHK(hipMemcpyAsync(&chol_failed, s->newton_fail, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->stats.host_syncs++;
    if (chol_failed)
        return fail(QN_ABNORMAL_TERMINATION, "the Hessian's Cholesky factorisation failed (its lower triangle is not positive definite): the reference "
                                             "unwraps here and there is no LU fallback; x is left at x_k");
    if (!small && s->pn_reuse && serial != 0) s->pn_factor_serial = serial;
    return QN_OK;
}

#define VEC_LAUNCH(kernel, grid)                                                                    \
    do {                                                                                            \
        ProfScope ps(s, KC_CTL);                                                                    \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(QN_VEC_TPB), 0, st, r.a);                       \
        s->stats.launches++;                                                                        \
        HIPCHK(hipGetLastError());                                                                  \
    } while (0)

static int vec_minimize(qn_solver* s, qn_linesearch* ls, const qn_oracle* o, size_t max_iter_solver, size_t max_iter_line_search,
                        qn_callback_fn callback, void* callback_user, int ls_only, double ls_f0) {
    qn_context* c = s->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (c->world > 1) return fail(QN_ERROR_INPUT_PARAMS, "SPG / projected gradient / projected Newton / L-BFGS / nonlinear CG run on one rank");
    const bool pn = pn_method(s->method), lbfgs = s->method == QN_LBFGS, cg = s->method == QN_NONLINEAR_CG, tn = s->method == QN_NEWTON_CG;
    const bool prox = s->method == QN_SPECTRAL_PROXIMAL_GRADIENT, owl = s->method == QN_OWLQN;
    VecRun r{s, o, nullptr, {}};
    QNCHK(check_oracle(c, s->n, o, &r.obj));
    if (prox) QNCHK(prox_check(s, ls, ls_only)); // GLLQuadratic or BackTracking, whole runs only
    if (owl) QNCHK(owl_check(s, ls, ls_only)); // BackTracking, whole runs, no box
    if (tn) QNCHK(tn_check(s, ls, r.obj, ls_only)); // unbounded, log-sum-exp, BackTracking or StrongWolfe without a box
    const bool exact = ls->kind == QN_LS_EXACT_QUADRATIC;
    if (exact) { // the exact step -g.d / d'Qd: a device quadratic under the four O(n) methods (qn_vec_exact.hip.h)
        if (pn) return fail(QN_ERROR_INPUT_PARAMS, "ExactQuadratic is not built for the projected Newton pair: it runs under SPG, projected gradient, L-BFGS and NonlinearCG");
        if (ls_only) return fail(QN_ERROR_INPUT_PARAMS, "ExactQuadratic: compute_step_len on its own is not built: use qn_minimize");
        if (!r.obj || !r.obj->ops->curvature)
            return fail(QN_ERROR_INPUT_PARAMS, "ExactQuadratic: the exact step needs a device quadratic (Quadratic or SparseQuadratic), not a closure or log-sum-exp");
        if (ls->lower_bound_host || ls->upper_bound_host)
            return fail(QN_ERROR_INPUT_PARAMS, "ExactQuadratic holds no box of its own: lower_bound_host / upper_bound_host must not be set (the solver's box caps the step at 1)");
        if (ls->_pad < 0) return fail(QN_ERROR_INPUT_PARAMS, "ExactQuadratic: refresh_every must not be negative");
    }
    if (cg) { // unbounded only: the searches that hold or imply a box, and the non-monotone one, are not this method's
        if (ls_only) return fail(QN_ERROR_INPUT_PARAMS, "compute_step_len runs on a first-order solver");
        if (ls->kind != QN_LS_STRONG_WOLFE && ls->kind != QN_LS_BACKTRACKING && !exact)
            return fail(QN_ERROR_INPUT_PARAMS, "NonlinearCG takes StrongWolfe or BackTracking, or ExactQuadratic on a device quadratic (GLLQuadratic, BackTrackingB and More-Thuente: out of scope)");
        if (ls->lower_bound_host || ls->upper_bound_host) return fail(QN_ERROR_INPUT_PARAMS, "NonlinearCG is unbounded only: StrongWolfe's box is out of scope");
        if (s->bounded) return fail(QN_ERROR_INPUT_PARAMS, "NonlinearCG is unbounded only");
    }
    if (ls->kind == QN_LS_MORETHUENTE || ls->kind == QN_LS_MORETHUENTE_B)
        return fail(QN_ERROR_INPUT_PARAMS, "More-Thuente with SPG / projected gradient / projected Newton / L-BFGS is out of scope: use GLLQuadratic, BackTracking or BackTrackingB");
    const bool wolfe = ls->kind == QN_LS_STRONG_WOLFE;
    if (ls->kind != QN_LS_GLL_QUADRATIC && ls->kind != QN_LS_BACKTRACKING && ls->kind != QN_LS_BACKTRACKING_B && !wolfe && !exact)
        return fail(QN_ERROR_INPUT_PARAMS, "unknown line search");
    if (wolfe) {
        if (ls_only) return fail(QN_ERROR_INPUT_PARAMS, "StrongWolfe: compute_step_len on its own is not built: use qn_minimize");
        if (!(ls->c1 > 0.0 && ls->c1 < ls->c2 && ls->c2 < 1.0)) return fail(QN_ERROR_INPUT_PARAMS, "StrongWolfe: 0 < c1 < c2 < 1");
        if (!(ls->delta >= 0.0)) return fail(QN_ERROR_INPUT_PARAMS, "StrongWolfe: xtol must not be negative");
        if (!(ls->t_min >= 0.0 && ls->t_max >= ls->t_min)) return fail(QN_ERROR_INPUT_PARAMS, "StrongWolfe: 0 <= t_min <= t_max");
    }
    // StrongWolfe holds a box of its own once one of its bounds is set, as the *_B searches do
    const bool wolfe_boxed = wolfe && (ls->lower_bound_host || ls->upper_bound_host);
    if (ls->kind == QN_LS_GLL_QUADRATIC && (ls->_pad < 1 || ls->_pad > QN_GLL_MAX_M))
        return fail(QN_ERROR_INPUT_PARAMS, "GLLQuadratic: the look-back m must be 1 .. 64 (the history is a fixed device ring)");
    if (pn) {
        if (ls_only) return fail(QN_ERROR_INPUT_PARAMS, "compute_step_len runs on a first-order solver");
        if (!(r.obj && !r.obj->ops->no_hessian && !r.obj->ops->hessian) && !(o->kind == QN_ORACLE_HOST && o->host_hessian_fn)) // (a device quadratic: its matrix is the Hessian)
            return fail(QN_ERROR_INPUT_PARAMS, "Hessian not available in the oracle"); // projected_newton.rs:73, spn.rs:85 .expect(...)
    }
    QNCHK(vec_state_alloc(s));
    if (exact) QNCHK(exact_state_alloc(s));
    hipStream_t st = c->stream;
    const size_t np = s->T.n_pad;
    if (ls->kind == QN_LS_BACKTRACKING_B || wolfe_boxed) {
        QNCHK(bounds_upload(s, s->bounds_block + 2 * np, ls->lower_bound_host, -INFINITY));
        QNCHK(bounds_upload(s, s->bounds_block + 3 * np, ls->upper_bound_host, INFINITY));
    }

    QnVecCtl* h = s->hvctl;
    h->tol = s->tol;
    h->max_iter = (int64_t)std::min<size_t>(max_iter_solver, (size_t)1 << 62);
    h->max_iter_ls = (int64_t)std::min<size_t>(max_iter_line_search, (size_t)1 << 62);
    h->method = s->method; h->ls_kind = ls->kind; h->memoize = o->memoize ? 1 : 0; h->ls_only = ls_only;
    if (ls->kind == QN_LS_GLL_QUADRATIC) { h->c1 = ls->c1; h->m = ls->_pad; h->sigma1 = ls->delta_min; h->sigma2 = ls->delta_max; h->beta = 0.0; }
    else if (wolfe) { h->c1 = ls->c1; h->w_c2 = ls->c2; h->w_xtol = ls->delta; h->w_tmin = ls->t_min; h->w_tmax = ls->t_max; h->beta = 0.0; h->m = 0; }
    else { h->c1 = ls->bt_c1; h->beta = ls->bt_beta; h->m = 0; }
    if (exact) { h->c1 = 0.0; h->beta = 0.0; h->m = 0; h->memoize = 1; } // (the accepted point's evaluation is always kept: memoize 0 and 1 run the same launches)
    h->ex_refresh_every = exact ? ls->_pad : 0; h->ex_err = 0; h->ex_adv = 0; h->ex_passes = 0; h->ex_refreshes = 0; h->ex_forced = 0;
    if (!exact) h->ex_g_true = 1; // (every other search's accepted gradient is the oracle's own: a memo it leaves behind is a true one)
    if (tn) { // the inner loop's cap for this call; the counters speak of this call
        h->tn_cap = h->tn_max_inner > 0 ? h->tn_max_inner : (int32_t)std::min<size_t>(s->n, 100);
        h->tn_state = 0; h->tn_inner_last = 0; h->tn_inner_total = 0; h->tn_hv_passes = 0; h->tn_neg_curv = 0; h->tn_fallbacks = 0;
        h->tn_diag_passes = 0; h->tn_floored_last = 0;
        QNCHK(tn_precond_alloc(s)); // (Jacobi: M and 1 / M, on first use)
    }
    uint64_t tn_weights = 0;
    h->w_boxed = wolfe_boxed ? 1 : 0; h->w_err = 0; h->tr_ls_cases = 0; h->tr_ndigits = 0;
    h->trace_cap = (int64_t)s->trace_cap; h->trace_x = s->trace_x;
    h->k = 0; h->ls_i = 0; h->status = -1; // ls_solver.rs:74
    h->n_calls = 0; h->n_evals = 0; h->n_iter = 0; h->tr_n_evals = 0; h->tr_ls_iters = 0;
    // the memo of the evaluation at x survives a call only on the same device objective, with nothing having touched x in between
    const uint64_t serial = r.obj ? r.obj->serial : 0;
    if (!(h->have_eval && h->memoize && s->hctl->have_cur_eval && serial != 0 && s->warm_obj == serial)) h->have_eval = 0;
    s->warm_obj = 0;
    bool done = false;
    if (ls_only) { h->f_cur = ls_f0; h->have_eval = 1; h->phase = QN_VP_LS_ONLY; }
    else if (spectral_method(s->method) && !h->has_lambda) h->phase = h->have_eval ? QN_VP_DIR : QN_VP_EVAL_X; // spg.rs:40-46, whatever the cap
    else if (h->max_iter <= 0) { h->status = QN_MAX_ITER_REACHED; h->phase = QN_VP_DONE; done = true; }  // ls_solver.rs:78
    else h->phase = h->have_eval ? QN_VP_DIR : QN_VP_EVAL_X;
    HIPCHK(hipMemcpyAsync(s->vctl, h, sizeof(QnVecCtl), hipMemcpyHostToDevice, st));
    if (done) HIPCHK(hipStreamSynchronize(st)); // (nothing else will wait for the upload: the host copy may be written again)

    QnVecArgs& a = r.a;
    a.x = s->V.x; a.g = s->V.g; a.d = s->V.d; a.xt = s->V.xt; a.gt = s->V.gt;
    a.lb = s->V.lb; a.ub = s->V.ub; a.llb = s->V.llb; a.lub = s->V.lub;
    a.z = s->V.y; a.part = s->vpart; a.ctl = s->vctl; a.f_dev = s->f_dev; a.trace = s->V.trace; a.xtrace = s->V.xtrace;
    a.n = (int)s->n; a.np = (int)np; a.G = vec_grid(np);
    a.cp = s->cg_p; a.cpart = s->cg_part;
    a.zw = s->V.y; a.lsmall = s->lb_small; // (the ring and the share buffer: lbfgs_enqueue_direction, on first use)
    const int G = a.G;
    const bool host_oracle = o->kind == QN_ORACLE_HOST;
    const size_t vb = np * sizeof(double);
    int64_t k_seen = 0, k_batch = 0;
    s->vec_d_searched = false;
    // qn_solver_get_direction / qn_solver_get_gradient (host flags only): a batch that accepted an iteration leaves the searched direction in V.d;
    // the memo flag is the batch's own, so that a callback reads what the run holds now
    auto batch_seen = [&]() { s->vec_d_searched = h->k != k_batch; k_batch = h->k; s->hctl->have_cur_eval = h->have_eval; };
    s->pn_factorisations = 0;
    // the run's bookkeeping, also when a batch fails after some iterations (a failed Cholesky, a closure's error): k, the counters, the
    // path and s_norm / y_norm speak of this call, not of the one before
    // s_norm() / y_norm() (projected_newton.rs:10-11) through the getters every solver answers: of the iteration just accepted, also inside
    // the callback (ls_solver.rs:105-107 hands the callback the solver behind update_next_iterate)
    auto publish_norms = [&]() {
        if (s->method == QN_PROJECTED_NEWTON) {
            s->hctl->has_s_norm = h->has_sy; s->hctl->has_y_norm = h->has_sy; s->hctl->s_norm = h->s_norm; s->hctl->y_norm = h->y_norm;
        }
    };
    auto epilogue = [&]() {
        s->hctl->k = h->k; s->hctl->n_iterations = h->n_iter; s->hctl->ls_result = h->ls_result;
        s->hctl->have_cur_eval = h->have_eval;
        s->warm_obj = (h->have_eval && h->memoize && serial != 0 && !ls_only) ? serial : 0;
        s->stats.iterations = h->n_iter;
        s->stats.oracle_calls = h->n_calls;
        s->stats.oracle_evals = h->n_evals;
        s->stats.h_passes = 0; s->stats.h_bytes = 0; s->stats.matrix_bytes_per_pass = 0;
        s->stats.obj_bytes = 0;
        if (r.obj) { // the kind's byte models: evaluations, ExactQuadratic's curvature passes, NewtonCG's products and weights passes
            const QnObjOps* ops = r.obj->ops;
            if (ops->vec_counted) s->stats.obj_bytes += h->n_evals * ops->eval_bytes(r.obj);
            if (exact) s->stats.obj_bytes += h->ex_passes * ops->curv_bytes(r.obj);
            if (tn) s->stats.obj_bytes += (uint64_t)h->tn_hv_passes * ops->hv_bytes(r.obj) + tn_weights * ops->weights_bytes(r.obj);
            if (tn && h->tn_precond) s->stats.obj_bytes += tn_weights * ops->diag_bytes(r.obj); // (one diagonal pass behind every weights pass)
        }
        stats_add_totals(s); // (no update passes, one rank: total_h_* and total_xchg_* stay)
        s->stats.path = QN_PATH_VECTOR | (pn ? QN_PATH_PNEWTON : 0u) | (lbfgs ? QN_PATH_LBFGS : 0u) | (cg ? QN_PATH_CG : 0u) | (exact ? QN_PATH_EXACT : 0u) | (tn ? QN_PATH_NEWTON_CG : 0u) | (prox ? QN_PATH_PROX : 0u) | (owl ? (QN_PATH_LBFGS | QN_PATH_OWLQN) : 0u);
        publish_norms();
    };

    while (!done) {
        int ph = h->phase;
        if (ph == QN_VP_EXACT_REFRESH) { // ExactQuadratic: the convergence test passed on a recurrence gradient; the objective evaluates x and the loop top runs again
            h->phase = ph = QN_VP_EVAL_X;
            HIPCHK(hipMemcpyAsync(s->vctl, h, sizeof(QnVecCtl), hipMemcpyHostToDevice, st));
        }
        // ExactQuadratic: does the objective evaluate the point this batch accepts?  exact_step_kernel applies the same rule to the same numbers (an
        // evaluation at x in this batch clears the count before it does)
        const int64_t ex_since = ph == QN_VP_EVAL_X ? 0 : h->ex_since;
        const bool ex_refresh = exact && (h->ex_refresh_every == 1 || (h->ex_refresh_every > 1 && ex_since + 1 >= (int64_t)h->ex_refresh_every));
        if (ph == QN_VP_EVAL_X) { // the oracle at x itself: through xt / gt like every evaluation
            HIPCHK(hipMemcpyAsync(s->V.xt, s->V.x, vb, hipMemcpyDeviceToDevice, st));
            if (host_oracle) {
                HIPCHK(hipMemcpyAsync(s->hx, s->V.x, s->n * sizeof(double), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                s->stats.host_syncs++;
            }
            QNCHK(vec_enqueue_eval(r));
            HIPCHK(hipMemcpyAsync(s->V.g, s->V.gt, vb, hipMemcpyDeviceToDevice, st));
        }
        if (ph == QN_VP_EVAL_X || ph == QN_VP_DIR || ph == QN_VP_LS_ONLY) {
            if (prox) { // prox_dir_kernel and prox_top_kernel in their places (qn_vec_prox.hip.h)
                QNCHK(prox_enqueue_direction(r));
            } else if (owl) { // the pseudo-gradient and the loop top, z = H_k v by L-BFGS's three kernels, the aligned direction and rule 3's test (qn_vec_owlqn.hip.h)
                QNCHK(owl_enqueue_direction(r));
            } else {
                VEC_LAUNCH(vec_dir_kernel, G);
                if (wolfe_boxed && !pn && !lbfgs) VEC_LAUNCH(wolfe_clip_kernel, G); // (those two form the direction the search follows in phase QN_VP_NSOLVE: the clip runs there)
                VEC_LAUNCH(vec_top_kernel, 1);
            }
            // the constructor's batch (spg.rs:40-46, spn.rs:40-46) ends here: no trial is wanted yet.  So does the second-order variants' loop top
            // when it ran as a batch of its own (the first iteration, or an oracle that is not memoised): the factorisation is enqueued only
            // for an iteration this peek has seen through the convergence test (QN_VP_NSOLVE)
            if ((spectral_method(s->method) && !h->has_lambda && !ls_only) || pn) {
                QNCHK(vec_peek(r, false));
                batch_seen();
                done = h->phase == QN_VP_DONE;
                continue;
            }
            // QN_LBFGS: gram, mid, apply, then the direction and the loop top's second half -- all predicated on QN_VP_NSOLVE, no peek in between
            if (lbfgs) QNCHK(lbfgs_enqueue_direction(r, wolfe_boxed));
            // QN_NONLINEAR_CG: the direction written directly, then the loop top's second half -- the same: one peek per batch
            if (cg) QNCHK(cg_enqueue_direction(r));
            // QN_NEWTON_CG: the weights at x, then a chunk of inner steps, the direction and the loop top's second half -- every one predicated: a
            // loop that outlasts the chunk leaves the phase at QN_VP_NSOLVE and the rest of this batch returns at once
            if (tn) QNCHK(tn_enqueue_direction(r, true, &tn_weights));
        } else if (ph == QN_VP_NSOLVE && pn) { // (QN_LBFGS never starts a batch here: no peek falls between its loop top and its direction)
            // the one n x n work matrix (Newton's), for the first iteration that wants a direction: a converged start, a cap of 0 and the
            // constructor's lambda0 batch never come here
            QNCHK(newton_alloc(s));
            const int rc = pn_enqueue_solve(r);
            if (rc != QN_OK) { // (the failing iteration's loop top ran: the control block on the host is that batch's, x is x_k)
                h->have_eval = 0; // the next call evaluates x_k afresh
                epilogue();
                return rc;
            }
            VEC_LAUNCH(vec_dir_kernel, G);
            if (wolfe_boxed) VEC_LAUNCH(wolfe_clip_kernel, G);
            VEC_LAUNCH(vec_top_kernel, 1);
        } else if (ph == QN_VP_NSOLVE && tn) { // the inner loop was still running when the last batch's chunk was used up: another chunk
            QNCHK(tn_enqueue_direction(r, false, &tn_weights));
        } else if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) {
            return fail(QN_ABNORMAL_TERMINATION, "vector pump: control block in an unexpected phase");
        }
        if (exact) { // the curvature pass and the step, then the accepted point's (f, g): the objective's launches or the recurrence, never both
            if (ph != QN_VP_TRIAL && ph != QN_VP_REEVAL) QNCHK(exact_enqueue_step(r));
            if (ex_refresh || ph == QN_VP_REEVAL) {
                VEC_LAUNCH(vec_trial_kernel, G);
                QNCHK(vec_enqueue_eval(r));
                VEC_LAUNCH(vec_decide_kernel, 1);
            } else {
                QNCHK(exact_enqueue_advance(r));
            }
            if (lbfgs) QNCHK(lbfgs_enqueue_accept(r));
            else if (cg) QNCHK(cg_enqueue_accept(r));
            else VEC_LAUNCH(vec_accept_kernel, G);
            VEC_LAUNCH(vec_post_kernel, 1);
            QNCHK(vec_peek(r, false));
            batch_seen();
            if (callback && h->k != k_seen) {
                k_seen = h->k;
                s->hctl->k = h->k; s->hctl->n_iterations = h->n_iter;
                publish_norms();
                callback(callback_user, s);
            }
            done = h->phase == QN_VP_DONE;
            continue;
        }
        if (prox) QNCHK(prox_enqueue_trial(r)); // xt and the shares of h(xt)
        else if (owl) QNCHK(owl_enqueue_trial(r)); // the projected xt and the shares of h(xt) and v.(xt - x)
        else VEC_LAUNCH(vec_trial_kernel, G);
        if (host_oracle) { // a host closure is called only for a point the machine asked for
            QNCHK(vec_peek(r, true));
            ph = h->phase;
            if (ph == QN_VP_TRIAL || ph == QN_VP_REEVAL) QNCHK(vec_enqueue_eval(r));
        } else {
            QNCHK(vec_enqueue_eval(r));
        }
        if (wolfe) { // phi'(t) = gt . d, then one dcsrch step in vec_decide_kernel's place (qn_vec_wolfe.hip.h)
            VEC_LAUNCH(wolfe_phi_kernel, G);
            VEC_LAUNCH(wolfe_decide_kernel, 1);
        } else if (prox) {
            QNCHK(prox_enqueue_decide(r)); // the same two branches on the composite values
        } else if (owl) {
            QNCHK(owl_enqueue_decide(r)); // Andrew and Gao's condition on the composite values
        } else {
            VEC_LAUNCH(vec_decide_kernel, 1);
        }
        if (lbfgs) QNCHK(lbfgs_enqueue_accept(r));
        else if (cg) QNCHK(cg_enqueue_accept(r));
        else if (owl) QNCHK(owl_enqueue_accept(r)); // x_next = xt, the projected point
        else VEC_LAUNCH(vec_accept_kernel, G);
        VEC_LAUNCH(vec_post_kernel, 1);
        QNCHK(vec_peek(r, false));
        batch_seen();
        if (callback && h->k != k_seen) { // ls_solver.rs:105-107: after k += 1 (one iteration per batch at most)
            k_seen = h->k;
            s->hctl->k = h->k; s->hctl->n_iterations = h->n_iter;
            publish_norms();
            callback(callback_user, s);
        }
        done = h->phase == QN_VP_DONE;
    }
    const int status = h->status;
    epilogue();
    if (status == QN_ABNORMAL_TERMINATION && h->w_err) // dcsrch's START errors; the loop top ran, x is x_k
        return fail(QN_ABNORMAL_TERMINATION, h->w_err == 1 ? "StrongWolfe: not a descent direction (g.d >= 0 at the start of the search); x is left at x_k"
                                                           : "StrongWolfe: not a descent direction the search can follow (the box leaves stpmax < stpmin); x is left at x_k");
    if (status == QN_ABNORMAL_TERMINATION && owl) // rule 3 is the only one that ends a run so: the loop top ran, x is x_k
        return fail(QN_ABNORMAL_TERMINATION, "OWLQN: not a descent direction (v.d is not < 0 after the alignment); x is left at x_k");
    if (status == QN_ABNORMAL_TERMINATION && h->ex_err) // the loop top ran, x is x_k
        return fail(QN_ABNORMAL_TERMINATION, h->ex_err == 1 ? "ExactQuadratic: not a descent direction (g.d >= 0 at the start of the search); x is left at x_k"
                                                            : "ExactQuadratic: non-positive curvature along the direction (d'Qd is not positive and finite); x is left at x_k");
    if (status < 0 || status == QN_ABNORMAL_TERMINATION) return fail(QN_ABNORMAL_TERMINATION, "vector pump: the machine stopped without a status");
    return status;
}

// qn_compute_step_len for GLLQuadratic: one compute_step_len on an empty f_previous (f_max = f_k)
static int vec_compute_step_len(qn_context* ctx, qn_linesearch* ls, const double* x_k_host, double f_k, const double* g_k_host,
                                const double* direction_host, size_t n, const qn_oracle* oracle, size_t max_iter, double* step_out) {
    qn_solver* s = nullptr;
    QNCHK(qn_solver_create(ctx, QN_PROJECTED_GRADIENT, 0.0, x_k_host, n, &s));
    int st = QN_OK;
    hipError_t e = hipMemcpyAsync(s->V.g, g_k_host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s->V.d, direction_host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) st = fail(QN_ABNORMAL_TERMINATION, std::string("compute_step_len upload: ") + hipGetErrorString(e));
    if (st == QN_OK) st = vec_minimize(s, ls, oracle, 1, max_iter, nullptr, nullptr, 1, f_k);
    if (st == QN_OK) *step_out = s->hvctl->ls_result;
    qn_solver_destroy(s);
    return st;
}
