// qn_vec_exact.hip.h -- the curvature pass of a device quadratic, q = Q v and c = v'Qv (public: qn_objective_hess_vec), and the ExactQuadratic line
// search (QN_LS_EXACT_QUADRATIC) that the first-order family's machine (qn_vec.hip.h) builds on it: the minimiser of a quadratic along d is
// t = -g.d / d'Qd, one product with Q, after which g(x + t d) = g + t q and f(x + t d) = f + t (g.d + (t / 2) d'Qd) need no second pass.
//
//   [vec_top_kernel]         its branch for this kind: g.d < 0 or the run ends; phase QN_VP_EXACT, no first trial of 1
//   the curvature pass       sparse: spq_curv_kernel<L> (qn_sparse.hip.h) -- spq_eval_kernel's structure, reading d for x and no b; q and the shares
//                            dense:  the row kernel of an evaluation with the point set to d (launch_quad_R, as vec_enqueue_eval launches it --
//                                    unconditional, like every evaluation of that objective: it writes scratch only), then quad_curv_finish_kernel in
//                                    quad_finish_kernel's place: q gathered, c = sum_i d_i q_i.  No new dense mat-vec.
//   exact_step_kernel        (1 workgroup) adds the sparse pass's shares in spq_finish_kernel's order (dense: reads c), then thread 0: c > 0 and
//                            finite or the run ends; t = (-g.d) / c; with a box t = min(t, 1); the refresh rule.  A refresh iteration goes on in phase
//                            QN_VP_REEVAL -- vec_trial_kernel, the objective's launches and vec_decide_kernel run as they do for every kind --, any
//                            other one is DECIDED HERE: f_t by the recurrence, gt_valid, the counters, phase QN_VP_ACCEPT.  (The one-workgroup decide
//                            of the recurrence is folded into this launch slot: one launch less per iteration.)
//   exact_advance_kernel     non-refresh iterations, in vec_trial_kernel's and the oracle's place: one stream of x, d, g, q (32 n read),
//                            xt = x + t d and gt = g + t q (16 n written), each with vec_trial_kernel's two roundings (the product first)
//   [the method's accept kernel, vec_post_kernel]   as for every kind
//
// CONVERGENCE IS DECLARED ONLY ON A TRUE GRADIENT (vec_loop_top): when the test passes on a recurrence gradient the machine parks in
// QN_VP_EXACT_REFRESH, which no kernel acts on, and the host starts the next batch in QN_VP_EVAL_X: the objective evaluates x, the loop top runs again.
//
// c's products and sums round separately (-ffp-contract=off), in fixed orders; reductions are two-stage; no atomic, no workgroup waits for another;
// every launch but the dense row kernel is predicated on the phase and the kind: the same bits from run to run and from object to object.
// Profiling mode: the curvature launch counts under t_newton_ms (no method that takes this search uses that class), exact_advance_kernel under
// t_ereduce_ms (unused by QN_NONLINEAR_CG, QN_SPG and QN_PROJECTED_GRADIENT; QN_LBFGS times its vec_dir_kernel there too), the rest under t_ctl_ms.
#pragma once

// `ctl` != NULL (the search): predicated on phase QN_VP_EXACT; NULL (qn_objective_hess_vec): unconditional
__global__ __launch_bounds__(QN_CTL_TPB) void quad_curv_finish_kernel(const QnVecs V, double* c_out, double* q_out, const QnVecCtl* ctl) {
    __shared__ double lds[16];
    if (ctl && ctl->phase != QN_VP_EXACT) return;
    double p[1] = {0.0};
    for (int i = threadIdx.x; i < V.n_pad; i += QN_CTL_TPB) {
        const double qi = q_val(V, i), vi = V.xt[i];
        p[0] = p[0] + vi * qi;
        q_out[i] = qi;
    }
    ctl_block_sum<1>(p, lds);
    if (threadIdx.x == 0) *c_out = p[0];
}

struct QnExactArgs {
    QnVecCtl* ctl;
    const double* part;  // the sparse pass's shares (NULL: a dense quadratic, c is in *c_dev)
    int count;
    const double* c_dev;
    int bounded;         // the solver has a box with a finite bound: d = P(x - z) - x, and t <= 1 keeps x + t d feasible
};

__global__ __launch_bounds__(SPQ_TPB) void exact_step_kernel(const QnExactArgs e) {
    __shared__ double lds[16];
    QnVecCtl* c = e.ctl;
    if (c->phase != QN_VP_EXACT || c->ls_kind != QN_LS_EXACT_QUADRATIC) return;
    double v[1] = {0.0};
    if (e.part) { // spq_finish_kernel's sum, operation for operation
        for (int b = threadIdx.x; b < e.count; b += SPQ_TPB) v[0] = v[0] + e.part[b];
        ctl_block_sum<1>(v, lds);
    }
    if (threadIdx.x != 0) return;
    const double cc = e.part ? v[0] : *e.c_dev;
    const double gd = c->gd;
    c->ex_c = cc;
    c->ex_passes++;
    if (!(cc > 0.0) || isinf(cc)) { c->ex_err = 2; c->status = QN_ABNORMAL_TERMINATION; c->phase = QN_VP_DONE; return; }
    double t = (-gd) / cc;
    if (e.bounded && t > 1.0) t = 1.0;
    c->t = t; c->ex_t = t; c->ls_result = t;
    const int r = c->ex_refresh_every;
    if (r == 1 || (r > 1 && c->ex_since + 1 >= (int64_t)r)) { // the objective evaluates x + t d: vec_trial_kernel, its launches, vec_decide_kernel
        c->ex_adv = 0; c->ex_since = 0; c->ex_g_true = 1; c->ex_refreshes++;
        c->gt_valid = 0;
        c->phase = QN_VP_REEVAL;
        return;
    }
    c->ex_adv = 1; c->ex_since++; c->ex_g_true = 0;
    const double half_t = 0.5 * t;
    const double inner = gd + half_t * cc;
    c->f_t = c->f_cur + t * inner;
    c->gt_valid = 1;
    c->n_calls++;
    c->phase = QN_VP_ACCEPT;
}

__global__ __launch_bounds__(QN_VEC_TPB) void exact_advance_kernel(const QnVecArgs a, const double* __restrict__ q) {
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_ACCEPT || c->ls_kind != QN_LS_EXACT_QUADRATIC || !c->ex_adv) return;
    const double t = c->t;
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), d = ld2(a.d + 2 * j), g = ld2(a.g + 2 * j), qq = ld2(q + 2 * j);
        const double td0 = t * d.x, td1 = t * d.y; // `t * direction_k` rounds first
        const double tq0 = t * qq.x, tq1 = t * qq.y;
        v2d u, w;
        u.x = x.x + td0;
        u.y = x.y + td1;
        w.x = g.x + tq0;
        w.y = g.y + tq1;
        st2(a.xt + 2 * j, u);
        st2(a.gt + 2 * j, w);
    }
}

extern "C" void qn_exact_quadratic_new(qn_linesearch* ls, int refresh_every) {
    memset(ls, 0, sizeof(*ls));
    ls->kind = QN_LS_EXACT_QUADRATIC;
    ls->_pad = refresh_every; // (a negative value is rejected by qn_minimize: this constructor returns nothing)
}

extern "C" int qn_solver_exact_state(qn_solver* s, size_t* curvature_passes, size_t* refreshes, double* last_t, double* last_curvature) {
    if (!s) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (!vec_method(s->method)) return fail(QN_ERROR_INPUT_PARAMS, "the ExactQuadratic search runs on SPG / projected gradient / L-BFGS / NonlinearCG solvers");
    const QnVecCtl* h = s->hvctl;
    if (curvature_passes) *curvature_passes = (size_t)h->ex_passes;
    if (refreshes) *refreshes = (size_t)h->ex_refreshes;
    if (last_t) *last_t = h->ex_t;
    if (last_curvature) *last_curvature = h->ex_c;
    return QN_OK;
}

// O(n): q of the last curvature pass (zeroed: the sparse pass writes entries 0 .. n only), and a dense quadratic's c
static int exact_state_alloc(qn_solver* s) {
    hipStream_t st = s->ctx->stream;
    QNCHK(s->ex_q.ensure(s->T.n_pad, st));
    QNCHK(s->ex_c.ensure(2, st));
    return QN_OK;
}

// the dense quadratic's curvature pass: q = Q d by the row kernel (which & 1), then d'Qd -> c_dev and q -> q_dev (which & 2).  `w`: as
// quad_enqueue_eval's; one rank
static int quad_enqueue_curvature(qn_objective* o, const double* d_dev, double* c_dev, double* q_dev, const QnVecCtl* ctl, int which, const QnObjWork* w) {
    QnVecs V{};
    double* xcopy = nullptr;
    QNCHK(quad_vecs(o, d_dev, w, &V, &xcopy));
    if (which & 1) QNCHK(quad_enqueue_rows(o, d_dev, V, xcopy));
    if (which & 2) hipLaunchKernelGGL(quad_curv_finish_kernel, dim3(1), dim3(QN_CTL_TPB), 0, o->ctx->stream, V, c_dev, q_dev, ctl);
    HIPCHK(hipGetLastError());
    return QN_OK;
}
static uint64_t quad_pass_bytes(const qn_objective* o) { return (uint64_t)o->T.rpr * (uint64_t)o->T.n_pad * 8ull; } // this rank's rows of Q, once

// the dense family evaluates a quadratic with kernels of its own (oracle_tpl = QN_ORACLE_QUAD); the first-order family and the host entry points use
// these.  One KC_EVAL scope for the two launches, as ever
static const QnObjOps kQuadOps = {
    /* eval */ quad_enqueue_eval, /* eval_launches */ 2, /* eval_split */ false, /* vec_counted */ true,
    /* weights */ nullptr, 0,
    /* hv_built, hess_vec, gbar, hv_out */ nullptr, nullptr, nullptr, nullptr, 0, false,
    /* curvature, curv_shares; hessian */ quad_enqueue_curvature, nullptr, nullptr, 0,
    /* bytes: eval, product, weights, curvature */ quad_pass_bytes, nullptr, nullptr, quad_pass_bytes,
    /* no_dense_family */ nullptr, /* no_rows */ nullptr, /* no_hessian */ nullptr, /* no_curvature */ nullptr,
};
static const QnObjOps* quad_ops() { return &kQuadOps; }

// phase QN_VP_EXACT: the curvature pass along V.d and the step, behind the loop top -- no peek in between
static int exact_enqueue_step(VecRun& r) {
    qn_solver* s = r.s;
    const QnObjOps* ops = r.obj->ops;
    QnExactArgs e{};
    e.ctl = s->vctl; e.c_dev = s->ex_c; e.bounded = (s->bounded && s->box_finite) ? 1 : 0;
    const QnObjWork w{s->V.q, s->V.s}; // (row-block 0 stores its copy of the point: V.s is free here)
    { ProfScope ps(s, KC_NEWTON); QNCHK(ops->curvature(r.obj, s->V.d, s->ex_c, s->ex_q, s->vctl, 1, &w)); }
    if (ops->curv_shares) { // exact_step_kernel adds the shares itself, in the finish kernel's order
        ops->curv_shares(r.obj, &e.part, &e.count);
        s->stats.launches += 1;
    } else {
        ProfScope ps(s, KC_CTL);
        QNCHK(ops->curvature(r.obj, s->V.d, s->ex_c, s->ex_q, s->vctl, 2, &w));
        s->stats.launches += 2;
    }
    ProfScope ps(s, KC_CTL);
    hipLaunchKernelGGL(exact_step_kernel, dim3(1), dim3(SPQ_TPB), 0, s->ctx->stream, e);
    HIPCHK(hipGetLastError());
    s->stats.launches++;
    return QN_OK;
}

// a non-refresh iteration: xt and gt by the recurrence (the step kernel has decided it: phase QN_VP_ACCEPT with ex_adv)
static int exact_enqueue_advance(VecRun& r) {
    qn_solver* s = r.s;
    ProfScope ps(s, KC_EREDUCE);
    hipLaunchKernelGGL(exact_advance_kernel, dim3(r.a.G), dim3(QN_VEC_TPB), 0, s->ctx->stream, r.a, (const double*)s->ex_q);
    HIPCHK(hipGetLastError());
    s->stats.launches++;
    return QN_OK;
}

extern "C" int qn_objective_hess_vec(qn_objective* o, const double* v_host, double* q_host, double* vqv) {
    if (!o || !v_host || !vqv) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (o->ops->no_curvature) return fail(QN_ERROR_INPUT_PARAMS, o->ops->no_curvature);
    qn_context* c = o->ctx;
    if (c->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "qn_objective_hess_vec is single-GPU");
    HIPCHK(hipSetDevice(c->device));
    const size_t np = o->T.n_pad;
    QNCHK(o->ex.ensure(2 * np, c->stream)); // v, and the row kernel's copy of the point
    QNCHK(o->eg.ensure(np, c->stream));
    QNCHK(o->ef.ensure(2, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex, v_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(o->ops->curvature(o, o->ex, o->ef, o->eg, nullptr, 3, nullptr));
    HIPCHK(hipMemcpyAsync(vqv, o->ef, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (q_host) HIPCHK(hipMemcpyAsync(q_host, o->eg, o->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return QN_OK;
}
