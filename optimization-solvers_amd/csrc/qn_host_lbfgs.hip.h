// qn_host_lbfgs.hip.h -- host side of QN_LBFGS (kernels: qn_lbfgs.hip.h; the pump is the first-order family's, qn_host_vec.hip.h): the memory's
// buffers, the setter and getter, and the two places where the pump enqueues this method's kernels.  The bookkeeping (pairs stored, head,
// gamma, resets) lives in QnVecCtl and travels with the pump's one small copy per batch; the vectors and the Gram matrices never leave the device.
#pragma once

// O(1): the small block (Gram matrices by slot, the coefficients).  Entries of slots that hold no live pair are never read.
static int lbfgs_state_alloc(qn_solver* s) {
    if (s->lb_small) return QN_OK;
    QNCHK(s->lb_small.alloc_zero(QN_LB_SMALL_LEN, s->ctx->stream));
    s->hvctl->lb_m = 5; // Lbfgsb::new, lbfgsb.rs:91
    s->hvctl->lb_gamma = 1.0;
    return QN_OK;
}

// O(m n): the ring of (lb_m + 1) slots for S and for Y, and the Gram kernel's shares -- made by the first qn_minimize that enqueues a direction
// (and made again when qn_solver_set_lbfgs_memory changed m: the memory is empty then)
static int lbfgs_ring_alloc(qn_solver* s) {
    const size_t np = s->T.n_pad, slots = (size_t)s->hvctl->lb_m + 1;
    hipStream_t st = s->ctx->stream;
    QNCHK(s->lb_ring.ensure(2 * slots * np, st));
    QNCHK(s->lb_part.ensure((size_t)QN_LBFGS_NQ * QN_VEC_MAXG, st));
    return QN_OK;
}

static int lbfgs_set_unit_scaling(qn_solver* s, bool on) { // QN_OPT_LBFGS_UNIT_SCALING
    s->hvctl->lb_unit = on ? 1 : 0;
    return QN_OK;
}

extern "C" int qn_solver_set_lbfgs_memory(qn_solver* s, size_t m) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_LBFGS && s->method != QN_OWLQN) return fail(QN_ERROR_INPUT_PARAMS, "the memory belongs to an L-BFGS or OWLQN solver");
    if (m < 1 || m > QN_LBFGS_MAX_M) return fail(QN_ERROR_INPUT_PARAMS, "L-BFGS: the memory m must be 1 .. 32 (the small solves run in one workgroup)");
    QnVecCtl* h = s->hvctl;
    h->lb_m = (int32_t)m;
    h->lb_kmem = 0; h->lb_head = 0; h->lb_gamma = 1.0; // the stored pairs are dropped (the slots are laid out for m + 1)
    return QN_OK;
}

extern "C" int qn_solver_lbfgs_state(qn_solver* s, size_t* m, size_t* stored, double* gamma, size_t* resets) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_LBFGS && s->method != QN_OWLQN) return fail(QN_ERROR_INPUT_PARAMS, "the memory belongs to an L-BFGS or OWLQN solver");
    const QnVecCtl* h = s->hvctl;
    if (m) *m = (size_t)h->lb_m;
    if (stored) *stored = (size_t)h->lb_kmem;
    if (gamma) *gamma = h->lb_gamma;
    if (resets) *resets = (size_t)h->lb_resets;
    return QN_OK;
}

// phase QN_VP_NSOLVE: z = H_k g into V.y by the two streams and the small kernel between them, then the direction and the rest of the loop top.
// The Gram kernel's second grid dimension comes from the host's copy of the pair count: it is the device's, because the only kernel that
// raises it (vec_post_kernel) runs in front of the batch's peek.
static int lbfgs_enqueue_direction(VecRun& r, bool wolfe_clip) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    QNCHK(lbfgs_ring_alloc(s));
    const size_t np = s->T.n_pad, slots = (size_t)s->hvctl->lb_m + 1;
    r.a.lS = s->lb_ring; r.a.lY = s->lb_ring + slots * np; r.a.lpart = s->lb_part;
    const int k = s->hvctl->lb_kmem;
    const int groups = std::max(1, (k + QN_LBFGS_GROUP - 1) / QN_LBFGS_GROUP);
    {
        ProfScope ps(s, KC_HPASS); // profiling mode, this method: t_hpass_ms = the Gram kernel, t_hreduce_ms = the apply kernel, t_ereduce_ms = vec_dir_kernel on z
        hipLaunchKernelGGL(lbfgs_gram_kernel, dim3(r.a.G, groups), dim3(QN_VEC_TPB), 0, st, r.a);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(s, KC_CTL);
        hipLaunchKernelGGL(lbfgs_mid_kernel, dim3(1), dim3(QN_VEC_TPB), 0, st, r.a);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(s, KC_HREDUCE);
        hipLaunchKernelGGL(lbfgs_apply_kernel, dim3(r.a.G), dim3(QN_VEC_TPB), 0, st, r.a);
        HIPCHK(hipGetLastError());
    }
    s->stats.launches += 3;
    {
        ProfScope ps(s, KC_EREDUCE);
        hipLaunchKernelGGL(vec_dir_kernel, dim3(r.a.G), dim3(QN_VEC_TPB), 0, st, r.a);
        HIPCHK(hipGetLastError());
    }
    if (wolfe_clip) { // StrongWolfe's boxed form: the ratio's minima behind the direction (qn_vec_wolfe.hip.h)
        ProfScope ps(s, KC_CTL);
        hipLaunchKernelGGL(wolfe_clip_kernel, dim3(r.a.G), dim3(QN_VEC_TPB), 0, st, r.a);
        HIPCHK(hipGetLastError());
        s->stats.launches++;
    }
    {
        ProfScope ps(s, KC_CTL);
        hipLaunchKernelGGL(vec_top_kernel, dim3(1), dim3(QN_VEC_TPB), 0, st, r.a);
        HIPCHK(hipGetLastError());
    }
    s->stats.launches += 2;
    return QN_OK;
}

static int lbfgs_enqueue_accept(VecRun& r) {
    qn_solver* s = r.s;
    QNCHK(lbfgs_ring_alloc(s)); // (a batch that starts in a trial phase: the ring exists already; this only fills the pointers)
    const size_t np = s->T.n_pad, slots = (size_t)s->hvctl->lb_m + 1;
    r.a.lS = s->lb_ring; r.a.lY = s->lb_ring + slots * np; r.a.lpart = s->lb_part;
    ProfScope ps(s, KC_CTL);
    hipLaunchKernelGGL(lbfgs_accept_kernel, dim3(r.a.G), dim3(QN_VEC_TPB), 0, s->ctx->stream, r.a);
    HIPCHK(hipGetLastError());
    s->stats.launches++;
    return QN_OK;
}
