// qn_host_logistic.hip.h -- host side of the logistic objective (kernels: qn_logistic.hip.h; the product's: qn_lse_hv.hip.h): the evaluation's two
// launches, the weights pass that leaves d at a point in `wp.w` for any number of Hessian-vector products, its operations table, and creation.
#pragma once

// enqueue one evaluation at x_dev (n_pad entries): f -> f_dev, g -> g_dev (n_pad entries, zero past n), d -> d_dev (m_pad entries; rows past m are
// never written).  `which`: 1 the stream of A, 2 the combine, 3 both (profiling mode times the two apart).
static int logit_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, double* d_dev, int which) {
    hipStream_t st = o->ctx->stream;
    const QnLseArgs a = dense_stream_args(o);
    int lst = QN_OK;
    if (which & 1) lst = lse_kch_call(o->os.kch, [&](auto K) { return logit_launch<decltype(K)::value>(st, o->os.G, a, x_dev, o->dn.rhs, d_dev, o->os.z, o->os.wgms, o->os.wgg); });
    QNCHK(lst);
    if (which & 2)
        hipLaunchKernelGGL(logit_combine_kernel, dim3((a.n_pad + 63) / 64), dim3(256), 0, st, a, o->os.G, (const double*)o->os.wgms, (const double*)o->os.wgg,
                           x_dev, f_dev, g_dev);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// the same stream of A at x_dev, leaving d in `wp.w` -- what the product reads until the next weights pass; its f and g go to scratch
static int logit_enqueue_weights(qn_objective* o, const double* x_dev) { return logit_enqueue_eval(o, x_dev, o->wp.scal, o->wp.g, o->wp.w, 3); }

// the table's evaluation: d goes to the trial buffer -- `wp.w` keeps the last weights pass's d, NewtonCG's at x_k
static int logit_eval_trial(qn_objective* o, const double* x, double* f, double* g, int which, const QnObjWork*) { return logit_enqueue_eval(o, x, f, g, o->wp.w_trial, which); }

// H = A' diag(d) A + mu I: the log-sum-exp product's kernels with pw = d and zeros where gbar goes.  One stream of A per evaluation, product, weights pass
static const QnObjOps kLogitOps = {
    /* eval */ logit_eval_trial, /* eval_launches */ 2, /* eval_split */ true, /* vec_counted */ true,
    /* weights */ logit_enqueue_weights, 2,
    /* hv_built, hess_vec, gbar, hv_out */ lse_hv_built, lse_enqueue_hess_vec, wp_zero_gbar, lse_hv_out, 2, false,
    /* curvature, curv_shares; hessian */ nullptr, nullptr, nullptr, 0,
    /* bytes: eval, product, weights, curvature */ dense_stream_bytes, dense_stream_bytes, dense_stream_bytes, nullptr,
    /* no_dense_family */ QN_VEC_FAMILY_ONLY("Logistic"),
    /* no_rows */ nullptr,
    /* no_hessian */ "the dense Hessian of a logistic objective is not built: hess_vec_at gives H(x) v in one stream of A",
    /* no_curvature */ "qn_objective_hess_vec: the Hessian of a logistic objective depends on x: use qn_objective_hess_vec_at",
    /* hess_diag, its launches and bytes */ dense_enqueue_hess_diag, 2, dense_stream_bytes,
};

// the device side of a new logistic objective: A, yw and every buffer the launches below use
static int logit_fill(qn_objective* o, const double* a_host, const double* yw_host) {
    const size_t n = o->n, m = o->dn.m, np = o->T.n_pad, mp = o->dn.TA.n_pad, mrpr = o->dn.TA.rpr;
    hipStream_t st = o->ctx->stream;
    QNCHK(o->dn.rows.alloc_zero(mrpr * np, st));
    QNCHK(o->dn.rhs.alloc_zero(mp, st));
    HIPCHK(hipMemcpyAsync(o->dn.rhs, yw_host, m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // the zero-fill above must land before the (null-stream) 2-D upload below
    HIPCHK(hipMemcpy2D(o->dn.rows, np * sizeof(double), a_host, n * sizeof(double), n * sizeof(double), std::min(mrpr, m), hipMemcpyHostToDevice));
    QNCHK(o->os.wgms.alloc_zero(2 * (size_t)o->os.G, st));    // per-workgroup F (the product's S)
    QNCHK(o->os.wgg.alloc_zero((size_t)o->os.G * np, st)); // per-workgroup G
    QNCHK(o->wp.w.alloc_zero(mp, st));                      // d at the accepted point (the product's pw)
    QNCHK(o->wp.w_trial.alloc_zero(mp, st));                // d of trial evaluations: never read
    QNCHK(o->wp.zero.alloc_zero(np, st));                   // the product's gbar slot
    QNCHK(o->os.z.alloc_zero(mp, st));                      // the margins of one stream of A: written and read inside its launch
    QNCHK(o->wp.g.alloc_zero(np, st));                  // g of a weights pass
    QNCHK(o->wp.scal.alloc_zero(2, st));                    // f of a weights pass
    HIPCHK(hipStreamSynchronize(st));
    return QN_OK;
}

// yw = y o w of the logistic pair, with the rules for labels and weights
static int logit_yw(size_t m, const double* y_host, const double* w_host, std::vector<double>& yw) {
    yw.resize(m);
    for (size_t i = 0; i < m; ++i) {
        if (y_host[i] != 1.0 && y_host[i] != -1.0)
            return fail(QN_ERROR_INPUT_PARAMS, "logistic: y[" + std::to_string(i) + "] is not -1 or +1 (labels are -1 / +1: pass 2 y - 1 for 0 / 1 labels)");
        const double w = w_host ? w_host[i] : 1.0;
        if (!(w >= 0.0) || !std::isfinite(w))
            return fail(QN_ERROR_INPUT_PARAMS, "logistic: weights[" + std::to_string(i) + "] is negative or not finite (a weight of 0 masks its row)");
        yw[i] = y_host[i] * w; // (+-w exactly; a masked row's entry is +-0, which every test in the kernel takes for 0)
    }
    return QN_OK;
}

extern "C" int qn_logistic_create(qn_context* ctx, size_t m, size_t n, const double* a_host, const double* y_host, const double* w_host, double mu,
                                  qn_objective** out) {
    if (!ctx || !out || !a_host || !y_host || n == 0 || m == 0) return fail(QN_ERROR_INPUT_PARAMS, "null argument or empty shape");
    if (n > (size_t)1 << 30 || m > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "shape too large");
    if (!std::isfinite(mu)) return fail(QN_ERROR_INPUT_PARAMS, "logistic: mu must be finite");
    if (ctx->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "the logistic objective is single-GPU (not built for a row-sharded context)");
    std::vector<double> yw;
    QNCHK(logit_yw(m, y_host, w_host, yw));
    const QnTile T = make_tile(n, ctx, 1), TA = make_tile(m, ctx, 1);
    if (T.n_pad > 16384) return fail(QN_ERROR_INPUT_PARAMS, "the logistic objective is not built for n_pad > 16384 (its evaluation keeps a whole row per workgroup in registers)");
    if (T.n_pad < 2) return fail(QN_ERROR_INPUT_PARAMS, "the logistic objective is not built for n_pad < 2");
    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    o->ctx = ctx; o->kind = OBJ_LOGISTIC; o->ops = &kLogitOps; o->n = n; o->dn.m = m; o->dn.mu = mu;
    o->T = T;   // column padding follows the solver's vectors
    o->dn.TA = TA; // the rows' padding (one rank owns them all)
    int kch = 1; // qn_logsumexp_create's rule
    while ((size_t)kch * 1024 < (size_t)T.n_pad) kch *= 2;
    o->os.kch = kch;
    o->os.G = (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)TA.rpr + 3) / 4));
    const int st = logit_fill(o, a_host, yw.data());
    if (st != QN_OK) { delete o; return st; } // (*out is written only for an objective that is whole: a failed allocation leaks nothing)
    *out = o;
    return QN_OK;
}
