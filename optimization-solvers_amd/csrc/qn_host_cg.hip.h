// qn_host_cg.hip.h -- host side of QN_NONLINEAR_CG (kernels: qn_cg.hip.h; the pump is the first-order family's, qn_host_vec.hip.h): the method's two
// buffers, the setter and getter, and the two places where the pump enqueues this method's kernels.  The bookkeeping (variant, beta, the counters,
// "p exists") lives in QnVecCtl and travels with the pump's one small copy per batch; the direction never leaves the device.
#pragma once

// O(n): the direction last searched and the accept kernel's shares.  Zeroed, though nothing reads p before cg_dir_kernel has written it (rule 1).
static int cg_state_alloc(qn_solver* s) {
    if (s->cg_p) return QN_OK;
    hipStream_t st = s->ctx->stream;
    QNCHK(s->cg_p.alloc_zero(s->T.n_pad, st));
    QNCHK(s->cg_part.alloc_zero((size_t)QN_CG_NQ * QN_VEC_MAXG, st));
    s->hvctl->cg_variant = QN_CG_PR_PLUS;
    s->hvctl->cg_powell_nu = 0.2;
    return QN_OK;
}

extern "C" int qn_solver_set_cg(qn_solver* s, int variant, double powell_nu, size_t restart_every) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_NONLINEAR_CG) return fail(QN_ERROR_INPUT_PARAMS, "the variant, Powell's nu and restart_every belong to a NonlinearCG solver");
    if (variant < QN_CG_FR || variant > QN_CG_HZ) return fail(QN_ERROR_INPUT_PARAMS, "NonlinearCG: unknown variant (QN_CG_FR, QN_CG_PR_PLUS, QN_CG_HS_PLUS, QN_CG_DY, QN_CG_HZ)");
    if (!(powell_nu > 0.0)) return fail(QN_ERROR_INPUT_PARAMS, "NonlinearCG: powell_nu must be positive (+inf disables Powell's restart test)");
    QnVecCtl* h = s->hvctl;
    h->cg_variant = variant;
    h->cg_powell_nu = powell_nu;
    h->cg_restart_every = (int64_t)std::min<size_t>(restart_every, (size_t)1 << 62);
    h->cg_has_p = 0; h->cg_beta = 0.0; h->cg_since = 0; // the stored direction is dropped: the next direction is -g
    return QN_OK;
}

extern "C" int qn_solver_cg_state(qn_solver* s, int* variant, double* beta, size_t* restarts, size_t* since_restart) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_NONLINEAR_CG) return fail(QN_ERROR_INPUT_PARAMS, "the variant, beta and the restart counters belong to a NonlinearCG solver");
    const QnVecCtl* h = s->hvctl;
    if (variant) *variant = h->cg_variant;
    if (beta) *beta = h->cg_beta;
    if (restarts) *restarts = (size_t)h->cg_restarts;
    if (since_restart) *since_restart = (size_t)h->cg_since;
    return QN_OK;
}

// phase QN_VP_NSOLVE: the direction and the rest of the loop top, behind the loop top's own two launches -- no peek in between
static int cg_enqueue_direction(VecRun& r) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    {
        ProfScope ps(s, KC_HPASS); // profiling mode, this method: t_hpass_ms = cg_dir_kernel, t_hreduce_ms = cg_accept_kernel
        hipLaunchKernelGGL(cg_dir_kernel, dim3(r.a.G), dim3(QN_VEC_TPB), 0, st, r.a);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(s, KC_CTL);
        hipLaunchKernelGGL(vec_top_kernel, dim3(1), dim3(QN_VEC_TPB), 0, st, r.a);
        HIPCHK(hipGetLastError());
    }
    s->stats.launches += 2;
    return QN_OK;
}

static int cg_enqueue_accept(VecRun& r) {
    qn_solver* s = r.s;
    ProfScope ps(s, KC_HREDUCE);
    hipLaunchKernelGGL(cg_accept_kernel, dim3(r.a.G), dim3(QN_VEC_TPB), 0, s->ctx->stream, r.a);
    HIPCHK(hipGetLastError());
    s->stats.launches++;
    return QN_OK;
}
