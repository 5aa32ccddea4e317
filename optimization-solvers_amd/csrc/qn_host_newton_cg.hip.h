// qn_host_newton_cg.hip.h -- host side of QN_NEWTON_CG (kernels: qn_newton_cg.hip.h, qn_lse_hv.hip.h; the pump is the first-order family's,
// qn_host_vec.hip.h): the method's buffers, the setter and getter, and the one place where the pump enqueues this method's launches.  The
// bookkeeping (the inner loop's scalars, the counters) lives in QnVecCtl and travels with the pump's one small copy per batch; z, r, p and q
// never leave the device, and no host read falls between the inner steps of a chunk.  The Jacobi preconditioner (qn_newton_cg.hip.h, rules 1' to 7')
// adds the objective's diagonal pass behind the weights and swaps init, update and next for their preconditioned siblings; without it nothing changes.
#pragma once

// O(n): r, p, q and the copy of gbar (z is the family's V.y), and the shares of the inner products (Jacobi: two more n-vectors, tn_precond_alloc)
static int tn_state_alloc(qn_solver* s) {
    if (s->tn_block) return QN_OK;
    hipStream_t st = s->ctx->stream;
    QNCHK(s->tn_block.alloc_zero(4 * (size_t)s->T.n_pad + (size_t)QN_TN_NPART * QN_VEC_MAXG, st));
    s->hvctl->tn_eta_max = 0.5;
    s->hvctl->tn_max_inner = 0;
    s->hvctl->tn_chunk = 8;
    s->hvctl->tn_precond = QN_PRECOND_NONE;
    return QN_OK;
}
// Jacobi: M = diag H(x_k) and 1 / M (zero-filled: the sparse kind's launch never writes entries n .. n_pad)
static int tn_precond_alloc(qn_solver* s) {
    if (!s->hvctl->tn_precond) return QN_OK;
    return s->tn_pc.ensure(2 * (size_t)s->T.n_pad, s->ctx->stream);
}

extern "C" int qn_solver_set_newton_cg_preconditioner(qn_solver* s, int kind) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_NEWTON_CG) return fail(QN_ERROR_INPUT_PARAMS, "the preconditioner belongs to a NewtonCG solver");
    if (kind != QN_PRECOND_NONE && kind != QN_PRECOND_JACOBI) return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG: the preconditioner is QN_PRECOND_NONE or QN_PRECOND_JACOBI");
    s->hvctl->tn_precond = kind;
    return QN_OK;
}

extern "C" int qn_solver_newton_cg_precond_state(qn_solver* s, int* kind, size_t* diag_passes, size_t* floored_last) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_NEWTON_CG) return fail(QN_ERROR_INPUT_PARAMS, "the preconditioner belongs to a NewtonCG solver");
    const QnVecCtl* h = s->hvctl;
    if (kind) *kind = h->tn_precond;
    if (diag_passes) *diag_passes = (size_t)h->tn_diag_passes;
    if (floored_last) *floored_last = (size_t)h->tn_floored_last;
    return QN_OK;
}

extern "C" int qn_solver_set_newton_cg(qn_solver* s, double eta_max, size_t max_inner, size_t chunk) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_NEWTON_CG) return fail(QN_ERROR_INPUT_PARAMS, "eta_max, max_inner and chunk belong to a NewtonCG solver");
    if (!(eta_max > 0.0 && eta_max < 1.0)) return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG: eta_max must lie in (0, 1)");
    if (chunk < 1) return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG: chunk must be at least 1");
    QnVecCtl* h = s->hvctl;
    h->tn_eta_max = eta_max;
    h->tn_max_inner = (int32_t)std::min<size_t>(max_inner, (size_t)1 << 30);
    h->tn_chunk = (int32_t)std::min<size_t>(chunk, (size_t)1 << 20);
    return QN_OK;
}

extern "C" int qn_solver_newton_cg_state(qn_solver* s, size_t* inner_last, size_t* inner_total, size_t* hv_passes, size_t* neg_curv, size_t* fallbacks) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_NEWTON_CG) return fail(QN_ERROR_INPUT_PARAMS, "the inner-loop counters belong to a NewtonCG solver");
    const QnVecCtl* h = s->hvctl;
    if (inner_last) *inner_last = (size_t)h->tn_inner_last;
    if (inner_total) *inner_total = (size_t)h->tn_inner_total;
    if (hv_passes) *hv_passes = (size_t)h->tn_hv_passes;
    if (neg_curv) *neg_curv = (size_t)h->tn_neg_curv;
    if (fallbacks) *fallbacks = (size_t)h->tn_fallbacks;
    return QN_OK;
}

extern "C" int qn_solver_newton_cg_precond_diag(qn_solver* s, double* m_host, double* minv_host) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_NEWTON_CG) return fail(QN_ERROR_INPUT_PARAMS, "the preconditioner belongs to a NewtonCG solver");
    if (!s->tn_pc) return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG: no run with the Jacobi preconditioner has been made");
    HIPCHK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (m_host) HIPCHK(hipMemcpyAsync(m_host, s->tn_pc, s->n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (minv_host) HIPCHK(hipMemcpyAsync(minv_host, s->tn_pc + s->T.n_pad, s->n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return QN_OK;
}

// what qn_minimize checks before a NewtonCG run starts (the pump's other checks have passed)
static int tn_check(const qn_solver* s, const qn_linesearch* ls, const qn_objective* obj, int ls_only) {
    if (ls_only) return fail(QN_ERROR_INPUT_PARAMS, "compute_step_len runs on a first-order solver");
    if (!obj) return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG needs a device LogSumExp or Logistic / SparseLogistic / Multinomial objective: a closure has no Hessian-vector product");
    if (!obj->ops->hess_vec)
        return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG runs on a LogSumExp or Logistic / SparseLogistic / Multinomial objective only: on a quadratic the method is linear conjugate gradients, which NonlinearCG with ExactQuadratic already is");
    if (ls->kind != QN_LS_BACKTRACKING && ls->kind != QN_LS_STRONG_WOLFE)
        return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG takes BackTracking or StrongWolfe (GLLQuadratic, BackTrackingB, ExactQuadratic, NoSearch and More-Thuente: out of scope)");
    if (ls->lower_bound_host || ls->upper_bound_host) return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG is unbounded only: StrongWolfe's box is out of scope");
    if (s->bounded) return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG is unbounded only");
    if (s->hvctl->tn_precond && !obj->ops->hess_diag)
        return fail(QN_ERROR_INPUT_PARAMS, "NewtonCG: the Jacobi preconditioner needs an objective with a Hessian diagonal (LogSumExp, Logistic, SparseLogistic)");
    return obj->ops->hv_built ? obj->ops->hv_built(obj) : QN_OK; // (log-sum-exp, logistic: n_pad <= 16384, one rank -- "not built" otherwise)
}

// phase QN_VP_NSOLVE.  fresh: behind the loop top's own two launches, in the batch that saw it pass -- the weights at x, init, start; then (and in
// a batch that starts in this phase because the loop was still running) `chunk` inner steps, the direction and the loop top's second half.  All
// predicated but the weights' launches, which write the objective's scratch only.  `weights_passes`: counted for qn_stats.obj_bytes.
static int tn_enqueue_direction(VecRun& r, bool fresh, uint64_t* weights_passes) {
    qn_solver* s = r.s;
    hipStream_t st = s->ctx->stream;
    const size_t np = s->T.n_pad;
    QnTnArgs t{};
    t.r = s->tn_block; t.p = s->tn_block + np; t.q = s->tn_block + 2 * np; t.gbar = s->tn_block + 3 * np; t.tpart = s->tn_block + 4 * np;
    const QnObjOps* ops = r.obj->ops;
    QnHvOut vhv{};
    QNCHK(ops->hv_out(r.obj, &vhv)); // the shares of v'Hv that tn_step_kernel adds, or the one value a kind folds itself
    t.gbar_src = ops->gbar(r.obj); t.kcount = vhv.count; t.kshares = vhv.shares;
    const dim3 one(1), wide(r.a.G), tpb(QN_VEC_TPB);
    const bool jacobi = s->hvctl->tn_precond != 0;
    if (jacobi) { t.mdiag = s->tn_pc; t.minv = s->tn_pc + np; }
    if (fresh) {
        {
            ProfScope ps(s, KC_EREDUCE); // (a class of its own: two passes of A, twice an evaluation's time, would upset t_eval_ms's floor rule)
            QNCHK(ops->weights(r.obj, s->V.x)); // unpredicated: it writes the objective's scratch only
            s->stats.launches += ops->weights_launches;
            ++*weights_passes;
            if (jacobi) { // rule 1': unpredicated as well -- the objective's scratch and the solver's M and 1 / M
                QNCHK(ops->hess_diag(r.obj, s->tn_pc, s->tn_pc + np));
                s->stats.launches += ops->diag_launches;
            }
        }
        if (jacobi) { ProfScope ps(s, KC_HPASS); hipLaunchKernelGGL(tn_pinit_kernel, wide, tpb, 0, st, r.a, t); }
        else { ProfScope ps(s, KC_HPASS); hipLaunchKernelGGL(tn_init_kernel, wide, tpb, 0, st, r.a, t); }
        { ProfScope ps(s, KC_CTL); hipLaunchKernelGGL(tn_start_kernel, one, tpb, 0, st, r.a, t); }
        HIPCHK(hipGetLastError());
        s->stats.launches += 2;
    }
    const int chunk = s->hvctl->tn_chunk;
    for (int i = 0; i < chunk; ++i) {
        { ProfScope ps(s, KC_NEWTON); QNCHK(ops->hess_vec(r.obj, t.p, t.gbar, t.q, s->vctl, 1)); }
        { ProfScope ps(s, ops->hv_fold_ctl ? KC_CTL : KC_NEWTON); QNCHK(ops->hess_vec(r.obj, t.p, t.gbar, t.q, s->vctl, 2)); }
        { ProfScope ps(s, KC_CTL); hipLaunchKernelGGL(tn_step_kernel, one, tpb, 0, st, r.a, t); }
        if (jacobi) { ProfScope ps(s, KC_HPASS); hipLaunchKernelGGL(tn_pupdate_kernel, wide, tpb, 0, st, r.a, t); }
        else { ProfScope ps(s, KC_HPASS); hipLaunchKernelGGL(tn_update_kernel, wide, tpb, 0, st, r.a, t); }
        { ProfScope ps(s, KC_CTL); hipLaunchKernelGGL(tn_commit_kernel, one, tpb, 0, st, r.a, t); }
        if (jacobi) { ProfScope ps(s, KC_HPASS); hipLaunchKernelGGL(tn_pnext_kernel, wide, tpb, 0, st, r.a, t); }
        else { ProfScope ps(s, KC_HPASS); hipLaunchKernelGGL(tn_next_kernel, wide, tpb, 0, st, r.a, t); }
        HIPCHK(hipGetLastError());
        s->stats.launches += 4 + ops->hv_launches;
    }
    { ProfScope ps(s, KC_HPASS); hipLaunchKernelGGL(tn_dir_kernel, wide, tpb, 0, st, r.a); }
    { ProfScope ps(s, KC_CTL); hipLaunchKernelGGL(tn_top_kernel, one, tpb, 0, st, r.a); }
    HIPCHK(hipGetLastError());
    s->stats.launches += 2;
    return QN_OK;
}
