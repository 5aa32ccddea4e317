// qn_host_prox.hip.h -- host side of QN_SPECTRAL_PROXIMAL_GRADIENT (kernels: qn_vec_prox.hip.h): the penalty's setter and getter, the
// refusals, and the three launches the pump of qn_host_vec.hip.h makes in vec_dir_kernel + vec_top_kernel's, vec_trial_kernel's and
// vec_decide_kernel's places.  The pump, its one peek per batch, the accept and the post kernel are SPG's.
#pragma once

static int prox_state_alloc(qn_solver* s) { // h0, Delta, F_k of the iteration being searched (+ 1 of padding)
    if (s->px_state) return QN_OK;
    QNCHK(s->px_state.alloc_zero(4, s->ctx->stream));
    return QN_OK;
}

extern "C" int qn_solver_set_l1(qn_solver* s, const double* l1_host, double l1_scalar) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_SPECTRAL_PROXIMAL_GRADIENT && s->method != QN_OWLQN) return fail(QN_ERROR_INPUT_PARAMS, "the L1 penalty belongs to a SpectralProximalGradient or OWLQN solver");
    if (l1_host) {
        for (size_t i = 0; i < s->n; ++i)
            if (!(l1_host[i] >= 0.0) || !std::isfinite(l1_host[i])) return fail(QN_ERROR_INPUT_PARAMS, "l1: every entry must be finite and not negative");
    } else if (!(l1_scalar >= 0.0) || !std::isfinite(l1_scalar)) {
        return fail(QN_ERROR_INPUT_PARAMS, "l1 must be finite and not negative");
    }
    HIPCHK(hipSetDevice(s->ctx->device));
    if (l1_host) {
        const size_t np = s->T.n_pad;
        if (!s->px_l1) QNCHK(s->px_l1.alloc_zero(np, s->ctx->stream)); // (entries n .. n_pad stay 0)
        s->px_l1_host.assign(l1_host, l1_host + s->n);
        HIPCHK(hipMemcpyAsync(s->px_l1, s->px_l1_host.data(), s->n * sizeof(double), hipMemcpyHostToDevice, s->ctx->stream));
        HIPCHK(hipStreamSynchronize(s->ctx->stream));
        s->px_l1_vec = true;
    } else {
        s->px_l1_host.clear();
        s->px_l1_scalar = l1_scalar;
        s->px_l1_vec = false;
    }
    // the ring's values belong to the old penalty; lambda, x and the memo (the smooth f and its gradient) do not
    // (QN_OWLQN keeps no such ring, and its pairs are differences of the smooth gradient: the memory is not touched)
    if (s->hvctl && s->method == QN_SPECTRAL_PROXIMAL_GRADIENT) s->hvctl->ring_len = 0;
    return QN_OK;
}

extern "C" int qn_solver_get_l1(qn_solver* s, double* l1_host) {
    if (!s || !l1_host) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_SPECTRAL_PROXIMAL_GRADIENT && s->method != QN_OWLQN) return fail(QN_ERROR_INPUT_PARAMS, "the L1 penalty belongs to a SpectralProximalGradient or OWLQN solver");
    for (size_t i = 0; i < s->n; ++i) l1_host[i] = s->px_l1_vec ? s->px_l1_host[i] : s->px_l1_scalar;
    return QN_OK;
}

// rule 4: GLLQuadratic and BackTracking; everything else is refused before any launch
static int prox_check(const qn_solver* s, const qn_linesearch* ls, int ls_only) {
    (void)s;
    if (ls_only) return fail(QN_ERROR_INPUT_PARAMS, "SpectralProximalGradient: compute_step_len on its own is not built: use qn_minimize");
    if (ls->kind != QN_LS_GLL_QUADRATIC && ls->kind != QN_LS_BACKTRACKING)
        return fail(QN_ERROR_INPUT_PARAMS, "SpectralProximalGradient takes GLLQuadratic or BackTracking (the composite decrease is built into those two; "
                                           "BackTrackingB, StrongWolfe, ExactQuadratic, More-Thuente and NoSearch: out of scope)");
    return QN_OK;
}

static QnProxArgs prox_args(const VecRun& r) {
    const qn_solver* s = r.s;
    QnProxArgs pa;
    pa.v = r.a;
    pa.l1 = s->px_l1_vec ? (const double*)s->px_l1 : nullptr;
    pa.l1s = s->px_l1_vec ? 0.0 : s->px_l1_scalar;
    pa.pst = s->px_state;
    return pa;
}

#define PROX_LAUNCH(kernel, grid)                                                                   \
    do {                                                                                            \
        ProfScope ps(s, KC_CTL);                                                                    \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(QN_VEC_TPB), 0, st, pa);                        \
        s->stats.launches++;                                                                        \
        HIPCHK(hipGetLastError());                                                                  \
    } while (0)

static int prox_enqueue_direction(VecRun& r) { // the instance is the solver's: a box once qn_solver_set_bounds was called, a vector once one was set
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    const QnProxArgs pa = prox_args(r);
    const int G = r.a.G;
    if (s->bounded) {
        if (s->px_l1_vec) PROX_LAUNCH((prox_dir_kernel<true, true>), G);
        else PROX_LAUNCH((prox_dir_kernel<true, false>), G);
    } else {
        if (s->px_l1_vec) PROX_LAUNCH((prox_dir_kernel<false, true>), G);
        else PROX_LAUNCH((prox_dir_kernel<false, false>), G);
    }
    PROX_LAUNCH(prox_top_kernel, 1);
    return QN_OK;
}
static int prox_enqueue_trial(VecRun& r) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    const QnProxArgs pa = prox_args(r);
    if (s->px_l1_vec) PROX_LAUNCH(prox_trial_kernel<true>, r.a.G);
    else PROX_LAUNCH(prox_trial_kernel<false>, r.a.G);
    return QN_OK;
}
static int prox_enqueue_decide(VecRun& r) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    const QnProxArgs pa = prox_args(r);
    PROX_LAUNCH(prox_decide_kernel, 1);
    return QN_OK;
}
