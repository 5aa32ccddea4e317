// qn_host_multinomial.hip.h -- host side of the multinomial objective (kernel: qn_multinomial.hip.h; the combines: qn_logistic.hip.h and qn_lse_hv.hip.h):
// the evaluation's two launches, the weights pass that leaves P at a point in `mn.P` for any number of Hessian-vector products, the product's two
// launches, its operations table, and creation.
#pragma once

// the automatic choice of the stream's kernel (DESIGN.md 30 has the measurement): the MFMA kernel where it is built and K fills more than one class tile
// of 16 -- at K = 64 it took 0.72 of the register-blocked kernel's time, at K <= 16 between 0.94 and 2.3 times it
static int mnl_auto_kernel(const qn_objective* o) { return o->mn.mfma.ok && o->mn.k > 16 ? 2 : 1; }

static QnMnlArgs mnl_args(const qn_objective* o, double* P, int product) {
    QnMnlArgs a{};
    a.A = o->dn.rows; a.wt = o->dn.rhs; a.lab = o->mn.lab; a.P = P;
    a.m = (int)o->dn.m; a.mrpr = o->dn.TA.rpr; a.nf = o->mn.nf; a.nfp = o->mn.nfp; a.K = o->mn.k; a.N = (int)o->n; a.N_pad = o->T.n_pad;
    a.tj_log2 = o->mn.plan.tj_log2; a.rt = o->mn.plan.RT; a.wk_log2 = o->mn.mfma.wk_log2; a.product = product;
    return a;
}

// the stream of A in the kernel the objective uses
static int mnl_launch_stream(qn_objective* o, const QnMnlArgs& a, const double* x_dev, const QnVecCtl* ctl) {
    if (o->mn.kernel == 2) return mnl_mfma_launch(o->ctx->stream, o->os.G, o->mn.mfma, a, x_dev, o->os.wgms, o->os.wgg, ctl);
    return mnl_launch(o->ctx->stream, o->os.G, o->mn.plan, a, x_dev, o->os.wgms, o->os.wgg, ctl);
}

// which kernel streams A: 1 mnl_onepass_kernel (register blocking on the vector unit: every shape), 2 mnl_mfma_kernel (v_mfma_f64_16x16x4_f64: K <= 64
// where its cut and its LDS fit, otherwise QN_ERROR_INPUT_PARAMS and nothing changes), 0 the automatic choice.  The two give different bits (another
// summation order), each its own from run to run; P of an earlier weights pass stays valid.
extern "C" int qn_multinomial_set_kernel(qn_objective* o, int kernel) {
    if (!o || o->kind != OBJ_MULTINOMIAL) return fail(QN_ERROR_INPUT_PARAMS, "not a multinomial objective");
    if (kernel < 0 || kernel > 2) return fail(QN_ERROR_INPUT_PARAMS, "multinomial: kernel must be 0 (automatic), 1 (vector unit) or 2 (MFMA)");
    if (kernel == 2 && !o->mn.mfma.ok) return fail(QN_ERROR_INPUT_PARAMS, "multinomial: the MFMA kernel is not built for this shape (K <= 64, at most 16 column tiles a wave, W and the rows' scratch in LDS)");
    o->mn.kernel = kernel == 0 ? mnl_auto_kernel(o) : kernel;
    return QN_OK;
}

// enqueue one evaluation at x_dev (N_pad entries): f -> f_dev, g -> g_dev (N_pad entries, zero past N), P -> p_dev (m_pad x K).
// `which`: 1 the stream of A, 2 the combine, 3 both (profiling mode times the two apart).
static int mnl_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, double* p_dev, int which) {
    hipStream_t st = o->ctx->stream;
    if (which & 1) QNCHK(mnl_launch_stream(o, mnl_args(o, p_dev, 0), x_dev, nullptr));
    if (which & 2) {
        const QnLseArgs a = dense_stream_args(o); // (the flat vector of N entries in N_pad)
        hipLaunchKernelGGL(logit_combine_kernel, dim3((a.n_pad + 63) / 64), dim3(256), 0, st, a, o->os.G, (const double*)o->os.wgms, (const double*)o->os.wgg,
                           x_dev, f_dev, g_dev);
    }
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// the same stream of A at x_dev, leaving P in `mn.P` -- what the product reads until the next weights pass; its f and g go to scratch
static int mnl_enqueue_weights(qn_objective* o, const double* x_dev) { return mnl_enqueue_eval(o, x_dev, o->wp.scal, o->wp.g, o->mn.P, 3); }

// enqueue q = H v into q_dev (N_pad entries, zero past N) and the shares of v'Hv into o->os.hv_shares, with P in o->mn.P (the combine
// takes wp.zero where gbar goes, whatever the unnamed argument is).  `ctl`, `which`: as lse_enqueue_hess_vec's
static int mnl_enqueue_hess_vec(qn_objective* o, const double* v_dev, const double*, double* q_dev, const QnVecCtl* ctl, int which) {
    hipStream_t st = o->ctx->stream;
    QNCHK(o->os.hv_shares.ensure(257, st));
    if (which & 1) QNCHK(mnl_launch_stream(o, mnl_args(o, o->mn.P, 1), v_dev, ctl));
    if (which & 2) {
        const QnLseArgs a = dense_stream_args(o); // (the flat vector of N entries in N_pad)
        hipLaunchKernelGGL(lse_hv_combine_kernel, dim3((a.n_pad + 63) / 64), dim3(256), 0, st, a, o->os.G, (const double*)o->os.wgms, (const double*)o->os.wgg,
                           v_dev, (const double*)o->wp.zero, q_dev, (double*)o->os.hv_shares, ctl);
    }
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// P at x (m x K, row-major) for the tests and for callers that want the class probabilities: one weights pass
extern "C" int qn_multinomial_probabilities(qn_objective* o, const double* x_host, double* p_host) {
    if (!o || o->kind != OBJ_MULTINOMIAL || !x_host || !p_host) return fail(QN_ERROR_INPUT_PARAMS, "not a multinomial objective, or a null argument");
    qn_context* c = o->ctx;
    HIPCHK(hipSetDevice(c->device));
    QNCHK(o->ex.ensure(2 * (size_t)o->T.n_pad, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(mnl_enqueue_weights(o, o->ex));
    HIPCHK(hipMemcpyAsync(p_host, o->mn.P, o->dn.m * (size_t)o->mn.k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return QN_OK;
}

// the table's evaluation: P goes to the trial buffer -- `mn.P` keeps the last weights pass's P, NewtonCG's at x_k
static int mnl_eval_trial(qn_objective* o, const double* x, double* f, double* g, int which, const QnObjWork*) { return mnl_enqueue_eval(o, x, f, g, o->mn.P_trial, which); }
// qn_stats.obj_bytes: A once, P once (written or read), the workgroups' shares -- per evaluation, product and weights pass
static uint64_t mnl_pass_bytes(const qn_objective* o) {
    return 8ull * ((uint64_t)o->dn.m * ((uint64_t)o->mn.nfp + (uint64_t)o->mn.k) + (uint64_t)o->os.G * (uint64_t)o->T.n_pad);
}

// H on the flat class-major vector: its own stream in product mode, the log-sum-exp product's combine (N_pad <= 16384 and one rank: checked at creation)
static const QnObjOps kMnlOps = {
    /* eval */ mnl_eval_trial, /* eval_launches */ 2, /* eval_split */ true, /* vec_counted */ true,
    /* weights */ mnl_enqueue_weights, 2,
    /* hv_built, hess_vec, gbar, hv_out */ nullptr, mnl_enqueue_hess_vec, wp_zero_gbar, lse_hv_out, 2, false,
    /* curvature, curv_shares; hessian */ nullptr, nullptr, nullptr, 0,
    /* bytes: eval, product, weights, curvature */ mnl_pass_bytes, mnl_pass_bytes, mnl_pass_bytes, nullptr,
    /* no_dense_family */ QN_VEC_FAMILY_ONLY("Multinomial"),
    /* no_rows */ "get_rows is not built for a multinomial objective (its n is K n_features, not the width of A)",
    /* no_hessian */ "the dense Hessian of a multinomial objective is not built: hess_vec_at gives H(x) v in one stream of A",
    /* no_curvature */ "qn_objective_hess_vec: the Hessian of a multinomial objective depends on x: use qn_objective_hess_vec_at",
};

// the device side of a new multinomial objective: A, the weights, the labels and every buffer the launches below use
static int mnl_fill(qn_objective* o, const double* a_host, const int* lab_host, const double* w_host) {
    const size_t nf = (size_t)o->mn.nf, nfp = (size_t)o->mn.nfp, m = o->dn.m, np = o->T.n_pad, mp = o->dn.TA.n_pad, mrpr = o->dn.TA.rpr, K = (size_t)o->mn.k;
    hipStream_t st = o->ctx->stream;
    QNCHK(o->dn.rows.alloc_zero(mrpr * nfp, st));
    QNCHK(o->dn.rhs.alloc_zero(mp, st));
    QNCHK(o->mn.lab.alloc(mp));
    HIPCHK(hipMemsetAsync(o->mn.lab, 0, mp * sizeof(int), st));
    HIPCHK(hipMemcpyAsync(o->dn.rhs, w_host, m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->mn.lab, lab_host, m * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // the zero-fill above must land before the (null-stream) 2-D upload below
    HIPCHK(hipMemcpy2D(o->dn.rows, nfp * sizeof(double), a_host, nf * sizeof(double), nf * sizeof(double), std::min(mrpr, m), hipMemcpyHostToDevice));
    QNCHK(o->os.wgms.alloc_zero(2 * (size_t)o->os.G, st));    // per-workgroup F (the product's S: zeros)
    QNCHK(o->os.wgg.alloc_zero((size_t)o->os.G * np, st));    // per-workgroup G, [workgroup][N_pad]
    QNCHK(o->mn.P.alloc_zero(mp * K, st));                   // P at the accepted point (what the product reads)
    QNCHK(o->mn.P_trial.alloc_zero(mp * K, st));             // P of trial evaluations: never read
    QNCHK(o->wp.zero.alloc_zero(np, st));                      // the product's gbar slot
    QNCHK(o->wp.g.alloc_zero(np, st));                     // g of a weights pass
    QNCHK(o->wp.scal.alloc_zero(2, st));                       // f of a weights pass
    HIPCHK(hipStreamSynchronize(st));
    return QN_OK;
}

extern "C" int qn_multinomial_create(qn_context* ctx, size_t m, size_t n, size_t k, const double* a_host, const void* labels_i32_host, const double* w_host,
                                     double mu, qn_objective** out) {
    const int32_t* labels_host = (const int32_t*)labels_i32_host;
    if (!ctx || !out || !a_host || !labels_host || n == 0 || m == 0) return fail(QN_ERROR_INPUT_PARAMS, "null argument or empty shape");
    if (k < 2) return fail(QN_ERROR_INPUT_PARAMS, "the multinomial objective is not built for fewer than 2 classes");
    if (n > (size_t)1 << 30 || m > (size_t)1 << 30 || k > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "shape too large");
    if (!std::isfinite(mu)) return fail(QN_ERROR_INPUT_PARAMS, "multinomial: mu must be finite");
    if (ctx->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "the multinomial objective is single-GPU (not built for a row-sharded context)");
    if (n * k > (size_t)16384) return fail(QN_ERROR_INPUT_PARAMS, "the multinomial objective is not built for a padded K n > 16384 (W stays on chip)");
    const QnTile T = make_tile(n * k, ctx, 1), TA = make_tile(m, ctx, 1), TF = make_tile(n, ctx, 1);
    if (T.n_pad > 16384) return fail(QN_ERROR_INPUT_PARAMS, "the multinomial objective is not built for a padded K n > 16384 (W stays on chip)");
    const QnMnlPlan plan = mnl_plan((int)n, (int)k);
    if (!plan.ok)
        return fail(QN_ERROR_INPUT_PARAMS, k > 256 ? "the multinomial objective is not built for more than 256 classes (a thread owns at most 32 classes of its column slots)"
                                                   : "the multinomial objective is not built for this shape: no cut of the workgroup holds W and the rows' scratch in LDS");
    std::vector<double> w(m);
    for (size_t i = 0; i < m; ++i) {
        if (labels_host[i] < 0 || (size_t)labels_host[i] >= k)
            return fail(QN_ERROR_INPUT_PARAMS, "multinomial: labels[" + std::to_string(i) + "] is outside [0, n_classes)");
        w[i] = w_host ? w_host[i] : 1.0;
        if (!(w[i] >= 0.0) || !std::isfinite(w[i]))
            return fail(QN_ERROR_INPUT_PARAMS, "multinomial: weights[" + std::to_string(i) + "] is negative or not finite (a weight of 0 masks its row)");
    }
    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    o->ctx = ctx; o->kind = OBJ_MULTINOMIAL; o->ops = &kMnlOps; o->n = n * k; o->dn.m = m; o->dn.mu = mu;
    o->T = T;   // the padding of the solver's vectors: N = K n entries
    o->dn.TA = TA; // the rows' padding (one rank owns them all)
    o->mn.k = (int)k; o->mn.nf = (int)n; o->mn.nfp = TF.n_pad; o->mn.plan = plan; o->mn.mfma = mnl_mfma_plan(TF.n_pad, (int)k); o->mn.kernel = mnl_auto_kernel(o);
    o->os.G = (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)TA.rpr + 3) / 4));
    const int st = mnl_fill(o, a_host, labels_host, w.data());
    if (st != QN_OK) { delete o; return st; } // (*out is written only for an objective that is whole: a failed allocation leaks nothing)
    *out = o;
    return QN_OK;
}
