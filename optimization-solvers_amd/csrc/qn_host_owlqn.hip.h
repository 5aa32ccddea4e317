// qn_host_owlqn.hip.h -- host side of QN_OWLQN (kernels: qn_vec_owlqn.hip.h): the method's buffers, the refusals, the pseudo-gradient's getter,
// and the launches the pump of qn_host_vec.hip.h makes in the direction's, the trial's, the decision's and the accept's places.  The penalty is
// SpectralProximalGradient's (qn_solver_set_l1, qn_host_prox.hip.h), the memory is L-BFGS's (qn_host_lbfgs.hip.h); the pump, its one peek per
// batch and the post kernel are the family's.
#pragma once

static int owl_state_alloc(qn_solver* s) { // the small block of the memory, h0 / v.d / F_k, and the pseudo-gradient: ONE n_pad vector beyond L-BFGS's
    QNCHK(lbfgs_state_alloc(s));
    QNCHK(prox_state_alloc(s));
    if (!s->ow_v) QNCHK(s->ow_v.alloc_zero(s->T.n_pad, s->ctx->stream));
    return QN_OK;
}

// rule 6: BackTracking on whole runs, no box, nothing else
static int owl_check(const qn_solver* s, const qn_linesearch* ls, int ls_only) {
    if (ls_only) return fail(QN_ERROR_INPUT_PARAMS, "OWLQN: compute_step_len on its own is not built: use qn_minimize");
    if (s->bounded) return fail(QN_ERROR_INPUT_PARAMS, "OWLQN is unbounded only (qn_solver_set_bounds was called): a box is out of scope");
    if (ls->kind != QN_LS_BACKTRACKING)
        return fail(QN_ERROR_INPUT_PARAMS, "OWLQN takes BackTracking only (the orthant projection is built into its trial; GLLQuadratic, BackTrackingB, "
                                           "StrongWolfe, ExactQuadratic, More-Thuente and NoSearch: out of scope)");
    return QN_OK;
}

extern "C" int qn_solver_get_pseudo_gradient(qn_solver* s, double* out_host) {
    if (!s || !out_host) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_OWLQN) return fail(QN_ERROR_INPUT_PARAMS, "the pseudo-gradient belongs to an OWLQN solver");
    HIPCHK(hipSetDevice(s->ctx->device));
    HIPCHK(hipMemcpyAsync(out_host, s->ow_v, s->n * sizeof(double), hipMemcpyDeviceToHost, s->ctx->stream));
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    return QN_OK;
}

static QnOwlArgs owl_args(const VecRun& r) {
    const qn_solver* s = r.s;
    QnOwlArgs oa;
    oa.v = r.a;
    oa.l1 = s->px_l1_vec ? (const double*)s->px_l1 : nullptr;
    oa.l1s = s->px_l1_vec ? 0.0 : s->px_l1_scalar;
    oa.pst = s->px_state;
    oa.pg = s->ow_v;
    return oa;
}

#define OWL_LAUNCH(kernel, grid, arg)                                                               \
    do {                                                                                            \
        ProfScope ps(s, KC_CTL);                                                                    \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(QN_VEC_TPB), 0, st, arg);                       \
        s->stats.launches++;                                                                        \
        HIPCHK(hipGetLastError());                                                                  \
    } while (0)

// pg, top | gram, mid, apply on a copy of the arguments whose g is v | dir, top: every one predicated, no peek in between
static int owl_enqueue_direction(VecRun& r) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    QNCHK(lbfgs_ring_alloc(s));
    const size_t np = s->T.n_pad, slots = (size_t)s->hvctl->lb_m + 1;
    r.a.lS = s->lb_ring; r.a.lY = s->lb_ring + slots * np; r.a.lpart = s->lb_part;
    const QnOwlArgs oa = owl_args(r);
    const int G = r.a.G;
    if (s->px_l1_vec) OWL_LAUNCH(owl_pg_kernel<true>, G, oa);
    else OWL_LAUNCH(owl_pg_kernel<false>, G, oa);
    OWL_LAUNCH(owl_top_kernel, 1, oa);
    QnVecArgs la = r.a; // z = H_k v: the three kernels read `g` and nothing else of the gradient
    la.g = s->ow_v;
    const int k = s->hvctl->lb_kmem; // (the device's: only vec_post_kernel raises it, in front of the batch's peek)
    const int groups = std::max(1, (k + QN_LBFGS_GROUP - 1) / QN_LBFGS_GROUP);
    {
        ProfScope ps(s, KC_HPASS);
        hipLaunchKernelGGL(lbfgs_gram_kernel, dim3(G, groups), dim3(QN_VEC_TPB), 0, st, la);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(s, KC_CTL);
        hipLaunchKernelGGL(lbfgs_mid_kernel, dim3(1), dim3(QN_VEC_TPB), 0, st, la);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(s, KC_HREDUCE);
        hipLaunchKernelGGL(lbfgs_apply_kernel, dim3(G), dim3(QN_VEC_TPB), 0, st, la);
        HIPCHK(hipGetLastError());
    }
    s->stats.launches += 3;
    if (s->px_l1_vec) OWL_LAUNCH(owl_dir_kernel<true>, G, oa);
    else OWL_LAUNCH(owl_dir_kernel<false>, G, oa);
    OWL_LAUNCH(owl_top_kernel, 1, oa);
    return QN_OK;
}
static int owl_enqueue_trial(VecRun& r) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    const QnOwlArgs oa = owl_args(r);
    if (s->px_l1_vec) OWL_LAUNCH(owl_trial_kernel<true>, r.a.G, oa);
    else OWL_LAUNCH(owl_trial_kernel<false>, r.a.G, oa);
    return QN_OK;
}
static int owl_enqueue_decide(VecRun& r) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    const QnOwlArgs oa = owl_args(r);
    OWL_LAUNCH(owl_decide_kernel, 1, oa);
    return QN_OK;
}
static int owl_enqueue_accept(VecRun& r) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    QNCHK(lbfgs_ring_alloc(s)); // (a batch that starts in a trial phase: the ring exists already; this only fills the pointers)
    const size_t np = s->T.n_pad, slots = (size_t)s->hvctl->lb_m + 1;
    r.a.lS = s->lb_ring; r.a.lY = s->lb_ring + slots * np; r.a.lpart = s->lb_part;
    OWL_LAUNCH(owl_accept_kernel, r.a.G, r.a);
    return QN_OK;
}
