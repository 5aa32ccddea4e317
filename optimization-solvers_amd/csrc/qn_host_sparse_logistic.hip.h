// qn_host_sparse_logistic.hip.h -- host side of the sparse logistic objective (kernels: qn_sparse_logistic.hip.h; the pure-host CSR code: qn_csr_host.h):
// the evaluation's three launches, the weights pass that leaves d at a point in `wp.w`, the product's three launches, its operations table, and creation.
#pragma once

#include "qn_csr_host.h"

// one CSR copy on the device, from its host arrays and its cut
static int slog_upload(QnSlogCsr& c, size_t rows, const std::vector<int>& rp, const std::vector<int>& ci, const double* val, size_t nnz,
                       const qn_csr::Cut& cut, hipStream_t st) {
    c.rows = rows; c.G = cut.G; c.n_long = (int)cut.longs.size(); c.lanes = c.lanes_auto = cut.lanes;
    QNCHK(c.row_ptr.alloc(rows + 1));
    QNCHK(c.col.alloc(std::max<size_t>(nnz, 1)));
    QNCHK(c.val.alloc_zero(std::max<size_t>(nnz, 1), st));
    QNCHK(c.cut.alloc((size_t)cut.G + 1));
    QNCHK(c.longs.alloc(std::max<size_t>(cut.longs.size(), 1)));
    QNCHK(c.part.alloc_zero((size_t)cut.G + cut.longs.size(), st));
    HIPCHK(hipMemcpyAsync(c.row_ptr, rp.data(), (rows + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c.col, ci.data(), std::max<size_t>(nnz, 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (nnz) HIPCHK(hipMemcpyAsync(c.val, val, nnz * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c.cut, cut.start.data(), cut.start.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!cut.longs.empty()) HIPCHK(hipMemcpyAsync(c.longs, cut.longs.data(), cut.longs.size() * sizeof(int), hipMemcpyHostToDevice, st));
    return QN_OK;
}

extern "C" int qn_sparse_logistic_set_lanes(qn_objective* o, int lanes_rows, int lanes_cols) {
    if (!o || o->kind != OBJ_SPARSE_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "lanes_rows / lanes_cols belong to a sparse logistic objective");
    for (int lanes : {lanes_rows, lanes_cols})
        if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1)) != 0)
            return fail(QN_ERROR_INPUT_PARAMS, "sparse logistic: lanes must be 0 (automatic), 1, 2, 4, 8, 16, 32 or 64");
    o->sl.a.lanes = lanes_rows ? lanes_rows : o->sl.a.lanes_auto;
    o->sl.at.lanes = lanes_cols ? lanes_cols : o->sl.at.lanes_auto;
    return QN_OK;
}

extern "C" int qn_sparse_logistic_info(qn_objective* o, size_t* nnz, int* lanes_rows, int* lanes_cols, size_t* n_long_rows, size_t* n_long_cols) {
    if (!o || o->kind != OBJ_SPARSE_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "not a sparse logistic objective");
    if (nnz) *nnz = o->sl.nnz;
    if (lanes_rows) *lanes_rows = o->sl.a.lanes;
    if (lanes_cols) *lanes_cols = o->sl.at.lanes;
    if (n_long_rows) *n_long_rows = (size_t)o->sl.a.n_long;
    if (n_long_cols) *n_long_cols = (size_t)o->sl.at.n_long;
    return QN_OK;
}

// the bytes one evaluation / one product moves by the model of qn_stats.obj_bytes: per pass 12 nnz + 4 (rows + 1), plus the vectors --
// evaluation: x, yw, coef, d (row pass), coef, x, g (column pass); product: v, d, t (row pass), t, v, q (column pass)
static uint64_t slog_eval_bytes(const qn_objective* o) {
    return 24ull * o->sl.nnz + 4ull * (o->sl.m + 1) + 4ull * (o->n + 1) + 32ull * o->sl.m + 24ull * o->n;
}
static uint64_t slog_product_bytes(const qn_objective* o) {
    return 24ull * o->sl.nnz + 4ull * (o->sl.m + 1) + 4ull * (o->n + 1) + 24ull * o->sl.m + 24ull * o->n;
}

static QnSlogArgs slog_args(const QnSlogCsr& c, double mu) {
    QnSlogArgs a{};
    a.row_ptr = c.row_ptr; a.col = c.col; a.val = c.val; a.wg_row_start = c.cut; a.long_rows = c.longs; a.part = c.part;
    a.mu = mu; a.G = c.G; a.n_long = c.n_long;
    return a;
}

// enqueue one evaluation at x_dev (n_pad entries): f -> f_dev, g -> g_dev[0 .. n), d -> d_dev (m entries).  `which`: 1 the two streaming launches
// (rows, then columns), 2 the finish, 3 all three (profiling mode times the two parts apart)
static int slog_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, double* d_dev, int which) {
    hipStream_t st = o->ctx->stream;
    if (which & 1) {
        QnSlogArgs r = slog_args(o->sl.a, o->sl.mu);
        r.src = x_dev; r.yw = o->sl.yw; r.out = o->sl.coef; r.d_out = d_dev;
        QNCHK((slog_launch<false, false>(st, r, o->sl.a.lanes, nullptr)));
        QnSlogArgs c = slog_args(o->sl.at, o->sl.mu);
        c.src = o->sl.coef; c.xv = x_dev; c.out = g_dev;
        QNCHK((slog_launch<false, true>(st, c, o->sl.at.lanes, nullptr)));
    }
    if (which & 2)
        hipLaunchKernelGGL(slog_finish_kernel, dim3(1), dim3(SPQ_TPB), 0, st, (const double*)o->sl.a.part, o->sl.a.G + o->sl.a.n_long,
                           (const double*)o->sl.at.part, o->sl.at.G + o->sl.at.n_long, o->sl.mu, f_dev, (const QnVecCtl*)nullptr, 0);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// the same three launches at x_dev, leaving d in `wp.w` -- what the products read until the next weights pass; f and g go to scratch
static int slog_enqueue_weights(qn_objective* o, const double* x_dev) { return slog_enqueue_eval(o, x_dev, o->wp.scal, o->wp.g, o->wp.w, 3); }

// enqueue q = H v into q_dev[0 .. n) with d from `wp.w`, and v'Hv folded into wp.scal[1] (no gbar: the unnamed argument).  `ctl`: the kernels' predicate
// (NULL: unconditional).
// `which`: 1 the two streaming launches, 2 the fold, 3 all three
static int slog_enqueue_hess_vec(qn_objective* o, const double* v_dev, const double*, double* q_dev, const QnVecCtl* ctl, int which) {
    hipStream_t st = o->ctx->stream;
    if (which & 1) {
        QnSlogArgs r = slog_args(o->sl.a, o->sl.mu);
        r.src = v_dev; r.d_in = o->wp.w; r.out = o->sl.t;
        QNCHK((slog_launch<true, false>(st, r, o->sl.a.lanes, ctl)));
        QnSlogArgs c = slog_args(o->sl.at, o->sl.mu);
        c.src = o->sl.t; c.xv = v_dev; c.out = q_dev;
        QNCHK((slog_launch<true, true>(st, c, o->sl.at.lanes, ctl)));
    }
    if (which & 2)
        hipLaunchKernelGGL(slog_finish_kernel, dim3(1), dim3(SPQ_TPB), 0, st, (const double*)nullptr, 0, (const double*)o->sl.at.part,
                           o->sl.at.G + o->sl.at.n_long, o->sl.mu, (double*)o->wp.scal + 1, ctl, 1);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// enqueue M = diag H(x) into m_dev[0 .. n) and, where minv_dev is not NULL, rule 2''s 1 / M into minv_dev[0 .. n), with d from `wp.w`: ONE launch
// over A', unpredicated.  Bytes by the model of qn_stats.obj_bytes: 12 nnz + 4 (n + 1) of A', d (8 m), M and 1 / M (16 n)
static int slog_enqueue_hess_diag(qn_objective* o, double* m_dev, double* minv_dev) {
    const QnSlogCsr& c = o->sl.at;
    QnSlogDiagArgs a{};
    a.row_ptr = c.row_ptr; a.col = c.col; a.val = c.val; a.wg_row_start = c.cut; a.long_rows = c.longs;
    a.d = o->wp.w; a.m_out = m_dev; a.minv_out = minv_dev; a.mu = o->sl.mu; a.G = c.G; a.n_long = c.n_long;
    QNCHK(slog_diag_launch(o->ctx->stream, a, c.lanes));
    HIPCHK(hipGetLastError());
    return QN_OK;
}
static uint64_t slog_diag_bytes(const qn_objective* o) { return 12ull * o->sl.nnz + 4ull * (o->n + 1) + 8ull * o->sl.m + 16ull * o->n; }

// the table's evaluation: d goes to the trial buffer, as the logistic's
static int slog_eval_trial(qn_objective* o, const double* x, double* f, double* g, int which, const QnObjWork*) { return slog_enqueue_eval(o, x, f, g, o->wp.w_trial, which); }
// v'Hv: one value, folded by the product's third launch
static int slog_hv_out(qn_objective* o, QnHvOut* out) { *out = QnHvOut{o->wp.scal + 1, 1, false}; return QN_OK; }

// kernels of its own for the product (no n_pad limit): rows, columns, then the fold, which is timed with the control kernels
static const QnObjOps kSlogOps = {
    /* eval */ slog_eval_trial, /* eval_launches */ 3, /* eval_split */ true, /* vec_counted */ true,
    /* weights */ slog_enqueue_weights, 3,
    /* hv_built, hess_vec, gbar, hv_out */ nullptr, slog_enqueue_hess_vec, wp_zero_gbar, slog_hv_out, 3, true,
    /* curvature, curv_shares; hessian */ nullptr, nullptr, nullptr, 0,
    /* bytes: eval, product, weights, curvature */ slog_eval_bytes, slog_product_bytes, slog_eval_bytes, nullptr,
    /* no_dense_family */ QN_VEC_FAMILY_ONLY("SparseLogistic"),
    /* no_rows */ "a sparse logistic objective has no dense rows / Hessian",
    /* no_hessian */ "a sparse logistic objective has no dense rows / Hessian: hess_vec_at gives H(x) v",
    /* no_curvature */ "qn_objective_hess_vec: the Hessian of a sparse logistic objective depends on x: use qn_objective_hess_vec_at",
    /* hess_diag, its launches and bytes */ slog_enqueue_hess_diag, 1, slog_diag_bytes,
};

// the device side of a new objective: both copies, yw and every buffer the launches below use.  The staging vectors live until the stream is idle.
static int slog_fill(qn_objective* o, const std::vector<int>& rp, const std::vector<int>& ci, const double* val, const double* yw_host) {
    const size_t n = o->n, m = o->sl.m, nnz = o->sl.nnz, np = o->T.n_pad;
    hipStream_t st = o->ctx->stream;
    std::vector<int> tp, tc;
    std::vector<double> tv;
    qn_csr::transpose(m, n, rp.data(), ci.data(), val, tp, tc, tv);
    const qn_csr::Cut ca = qn_csr::cut(m, rp.data(), SPQ_MAXG, SPQ_LONG_ROW), cat = qn_csr::cut(n, tp.data(), SPQ_MAXG, SPQ_LONG_ROW);
    int status = slog_upload(o->sl.a, m, rp, ci, val, nnz, ca, st);
    if (status == QN_OK) status = slog_upload(o->sl.at, n, tp, tc, tv.data(), nnz, cat, st);
    if (status == QN_OK) status = o->sl.yw.alloc_zero(m, st);          // yw = y o w
    if (status == QN_OK) status = o->sl.coef.alloc_zero(m, st);    // -(yw s) of one evaluation: written by its row pass, gathered by its column pass
    if (status == QN_OK) status = o->sl.t.alloc_zero(m, st);       // d o (A v) of one product
    if (status == QN_OK) status = o->wp.w.alloc_zero(m, st);         // d at the accepted point (what the products read)
    if (status == QN_OK) status = o->wp.w_trial.alloc_zero(m, st);   // d of trial evaluations: never read
    if (status == QN_OK) status = o->wp.zero.alloc_zero(np, st);     // NewtonCG's gbar slot
    if (status == QN_OK) status = o->wp.g.alloc_zero(np, st);    // g of a weights pass
    if (status == QN_OK) status = o->wp.scal.alloc_zero(2, st);      // f of a weights pass; v'Hv of a product
    if (status == QN_OK && hipMemcpyAsync(o->sl.yw, yw_host, m * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
        status = fail(QN_ABNORMAL_TERMINATION, "sparse logistic: the upload of y o w failed");
    const hipError_t e = hipStreamSynchronize(st); // (also after a failure: the copies enqueued so far read the vectors above)
    if (status == QN_OK && e != hipSuccess) status = fail(QN_ABNORMAL_TERMINATION, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return status;
}

extern "C" int qn_sparse_logistic_create(qn_context* ctx, size_t m, size_t n, size_t nnz, const void* row_ptr_host, const void* col_idx_host,
                                         int index_bytes, const double* values_host, const double* y_host, const double* w_host, double mu,
                                         qn_objective** out) {
    if (!ctx || !out || !row_ptr_host || !col_idx_host || !values_host || !y_host || n == 0 || m == 0)
        return fail(QN_ERROR_INPUT_PARAMS, "null argument or empty shape");
    if (index_bytes != 4 && index_bytes != 8) return fail(QN_ERROR_INPUT_PARAMS, "sparse logistic: index_bytes must be 4 or 8");
    if (n > (size_t)1 << 30 || m > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "shape too large");
    if (nnz > (size_t)INT32_MAX) return fail(QN_ERROR_INPUT_PARAMS, "sparse logistic: nnz must not exceed 2^31 - 1");
    if (!std::isfinite(mu)) return fail(QN_ERROR_INPUT_PARAMS, "logistic: mu must be finite");
    if (ctx->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "the sparse logistic objective is single-GPU (it lives on one rank: no row sharding)");
    std::vector<double> yw;
    QNCHK(logit_yw(m, y_host, w_host, yw)); // qn_logistic_create's rules
    std::string err;
    const bool ok = index_bytes == 4 ? qn_csr::validate(m, n, nnz, (const int32_t*)row_ptr_host, (const int32_t*)col_idx_host, &err)
                                     : qn_csr::validate(m, n, nnz, (const int64_t*)row_ptr_host, (const int64_t*)col_idx_host, &err);
    if (!ok) return fail(QN_ERROR_INPUT_PARAMS, "sparse logistic: " + err);
    std::vector<int> rp, ci;
    if (index_bytes == 4) qn_csr::narrow(m, nnz, (const int32_t*)row_ptr_host, (const int32_t*)col_idx_host, rp, ci);
    else qn_csr::narrow(m, nnz, (const int64_t*)row_ptr_host, (const int64_t*)col_idx_host, rp, ci);
    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    o->ctx = ctx; o->kind = OBJ_SPARSE_LOGISTIC; o->ops = &kSlogOps; o->n = n; o->sl.m = m; o->sl.mu = mu; o->sl.nnz = nnz;
    o->T = make_tile(n, ctx, 1); // (the padding of the solver's vectors)
    const int st = slog_fill(o, rp, ci, values_host, yw.data());
    if (st != QN_OK) { delete o; return st; } // (*out is written only for an objective that is whole: a failed creation leaks nothing)
    *out = o;
    return QN_OK;
}
