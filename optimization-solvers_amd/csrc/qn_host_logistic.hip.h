// qn_host_logistic.hip.h -- host side of the logistic objective (kernels: qn_logistic.hip.h; the product's: qn_lse_hv.hip.h): creation and validation,
// the evaluation's two launches, and the weights pass that leaves d at a point in `lw` for any number of Hessian-vector products.
#pragma once

// the device side of a new logistic objective: A, yw and every buffer the launches below use
static int logit_fill(qn_objective* o, const double* a_host, const double* yw_host) {
    const size_t n = o->n, m = o->m, np = o->T.n_pad, mp = o->TA.n_pad, mrpr = o->TA.rpr;
    hipStream_t st = o->ctx->stream;
    QNCHK(o->Q.alloc_zero(mrpr * np, st));
    QNCHK(o->b.alloc_zero(mp, st));
    HIPCHK(hipMemcpyAsync(o->b, yw_host, m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // the zero-fill above must land before the (null-stream) 2-D upload below
    HIPCHK(hipMemcpy2D(o->Q, np * sizeof(double), a_host, n * sizeof(double), n * sizeof(double), std::min(mrpr, m), hipMemcpyHostToDevice));
    QNCHK(o->lwgms.alloc_zero(2 * (size_t)o->lse_G, st));    // per-workgroup F (the product's S)
    QNCHK(o->lwgg.alloc_zero((size_t)o->lse_G * np, st)); // per-workgroup G
    QNCHK(o->lw.alloc_zero(mp, st));                      // d at the accepted point (the product's pw)
    QNCHK(o->lw_trial.alloc_zero(mp, st));                // d of trial evaluations: never read
    QNCHK(o->lzero.alloc_zero(np, st));                   // the product's gbar slot
    QNCHK(o->lz.alloc_zero(mp, st));                      // the margins of one stream of A: written and read inside its launch
    QNCHK(o->lgpart.alloc_zero(np, st));                  // g of a weights pass
    QNCHK(o->lscal.alloc_zero(2, st));                    // f of a weights pass
    HIPCHK(hipStreamSynchronize(st));
    return QN_OK;
}

extern "C" int qn_logistic_create(qn_context* ctx, size_t m, size_t n, const double* a_host, const double* y_host, const double* w_host, double mu,
                                  qn_objective** out) {
    if (!ctx || !out || !a_host || !y_host || n == 0 || m == 0) return fail(QN_ERROR_INPUT_PARAMS, "null argument or empty shape");
    if (n > (size_t)1 << 30 || m > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "shape too large");
    if (!std::isfinite(mu)) return fail(QN_ERROR_INPUT_PARAMS, "logistic: mu must be finite");
    if (ctx->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "the logistic objective is single-GPU (not built for a row-sharded context)");
    std::vector<double> yw(m);
    for (size_t i = 0; i < m; ++i) {
        if (y_host[i] != 1.0 && y_host[i] != -1.0)
            return fail(QN_ERROR_INPUT_PARAMS, "logistic: y[" + std::to_string(i) + "] is not -1 or +1 (labels are -1 / +1: pass 2 y - 1 for 0 / 1 labels)");
        const double w = w_host ? w_host[i] : 1.0;
        if (!(w >= 0.0) || !std::isfinite(w))
            return fail(QN_ERROR_INPUT_PARAMS, "logistic: weights[" + std::to_string(i) + "] is negative or not finite (a weight of 0 masks its row)");
        yw[i] = y_host[i] * w; // (+-w exactly; a masked row's entry is +-0, which every test in the kernel takes for 0)
    }
    const QnTile T = make_tile(n, ctx, 1), TA = make_tile(m, ctx, 1);
    if (T.n_pad > 16384) return fail(QN_ERROR_INPUT_PARAMS, "the logistic objective is not built for n_pad > 16384 (its evaluation keeps a whole row per workgroup in registers)");
    if (T.n_pad < 2) return fail(QN_ERROR_INPUT_PARAMS, "the logistic objective is not built for n_pad < 2");
    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    o->ctx = ctx; o->kind = OBJ_LOGISTIC; o->n = n; o->m = m; o->mu = mu;
    o->T = T;   // column padding follows the solver's vectors
    o->TA = TA; // the rows' padding (one rank owns them all)
    int kch = 1; // qn_logsumexp_create's rule
    while ((size_t)kch * 1024 < (size_t)T.n_pad) kch *= 2;
    o->lse_kch = kch;
    o->lse_G = (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)TA.rpr + 3) / 4));
    const int st = logit_fill(o, a_host, yw.data());
    if (st != QN_OK) { delete o; return st; } // (*out is written only for an objective that is whole: a failed allocation leaks nothing)
    *out = o;
    return QN_OK;
}

// enqueue one evaluation at x_dev (n_pad entries): f -> f_dev, g -> g_dev (n_pad entries, zero past n), d -> d_dev (m_pad entries; rows past m are
// never written).  `which`: 1 the stream of A, 2 the combine, 3 both (profiling mode times the two apart).
static int logit_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, double* d_dev, int which) {
    hipStream_t st = o->ctx->stream;
    QnLseArgs a{};
    a.A = o->Q; a.mu = o->mu;
    a.m = (int)o->m; a.m_pad = o->TA.n_pad; a.mrpr = o->TA.rpr; a.n = (int)o->n; a.n_pad = o->T.n_pad;
    a.world = 1; a.rank = 0; a.rs = 1;
    int lst = QN_OK;
    if (which & 1) switch (o->lse_kch) {
    case 1: lst = logit_launch<1>(st, o->lse_G, a, x_dev, o->b, d_dev, o->lz, o->lwgms, o->lwgg); break;
    case 2: lst = logit_launch<2>(st, o->lse_G, a, x_dev, o->b, d_dev, o->lz, o->lwgms, o->lwgg); break;
    case 4: lst = logit_launch<4>(st, o->lse_G, a, x_dev, o->b, d_dev, o->lz, o->lwgms, o->lwgg); break;
    case 8: lst = logit_launch<8>(st, o->lse_G, a, x_dev, o->b, d_dev, o->lz, o->lwgms, o->lwgg); break;
    default: lst = logit_launch<16>(st, o->lse_G, a, x_dev, o->b, d_dev, o->lz, o->lwgms, o->lwgg); break;
    }
    QNCHK(lst);
    if (which & 2)
        hipLaunchKernelGGL(logit_combine_kernel, dim3((a.n_pad + 63) / 64), dim3(256), 0, st, a, o->lse_G, (const double*)o->lwgms, (const double*)o->lwgg,
                           x_dev, f_dev, g_dev);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// the same stream of A at x_dev, leaving d in `lw` -- what the product reads until the next weights pass; its f and g go to scratch
static int logit_enqueue_weights(qn_objective* o, const double* x_dev) { return logit_enqueue_eval(o, x_dev, o->lscal, o->lgpart, o->lw, 3); }

// H(x) v for qn_objective_hess_vec_at: one weights pass, one product, the shares' sum
static int logit_hess_vec_at(qn_objective* o, const double* x_host, const double* v_host, double* q_host, double* vhv) {
    qn_context* c = o->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t np = o->T.n_pad;
    QNCHK(o->ex.ensure(2 * np, c->stream)); // x, then v
    QNCHK(o->eg.ensure(np, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex + np, v_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(logit_enqueue_weights(o, o->ex));
    QNCHK(lse_enqueue_hess_vec(o, o->ex + np, o->lzero, o->eg, nullptr));
    const int count = (int)((np + 63) / 64);
    hipLaunchKernelGGL(lse_hv_shares_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)o->lhv_shares, count, (double*)o->lhv_shares + 256);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(vhv, o->lhv_shares + 256, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (q_host) HIPCHK(hipMemcpyAsync(q_host, o->eg, o->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return QN_OK;
}
