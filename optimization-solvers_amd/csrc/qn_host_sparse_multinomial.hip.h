// qn_host_sparse_multinomial.hip.h -- host side of the sparse multinomial objective (kernels: qn_sparse_multinomial.hip.h; the pure-host CSR code:
// qn_csr_host.h; the upload of a CSR copy: qn_host_sparse_logistic.hip.h): the evaluation's five launches, the weights pass that leaves P at a point
// in `sm.P` for any number of products, the product's five launches, its operations table, and creation.
#pragma once

#include "qn_csr_host.h"

// the automatic entry lanes of a copy: SparseQuadratic's rule for the mean row length, capped at 16 lanes per row, class lanes included -- measured
// (tools/bench_sparse_multinomial.py --lanes): at 16 per row and K = 16, L = 1 beat L = 4 by 20 %; at K = 4, L = 2 and 4 beat 1 and 8
static int smn_auto_lanes(int cut_lanes, int K) { return std::max(1, std::min(cut_lanes, 16 / smn_cl(K, 1))); }

extern "C" int qn_sparse_multinomial_set_lanes(qn_objective* o, int lanes_rows, int lanes_cols) {
    if (!o || o->kind != OBJ_SPARSE_MULTINOMIAL) return fail(QN_ERROR_INPUT_PARAMS, "lanes_rows / lanes_cols belong to a sparse multinomial objective");
    for (int lanes : {lanes_rows, lanes_cols})
        if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1)) != 0)
            return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: lanes must be 0 (automatic), 1, 2, 4, 8, 16, 32 or 64");
    o->sm.a.lanes = lanes_rows ? lanes_rows : o->sm.a.lanes_auto;
    o->sm.at.lanes = lanes_cols ? lanes_cols : o->sm.at.lanes_auto;
    return QN_OK;
}

extern "C" int qn_sparse_multinomial_info(qn_objective* o, size_t* nnz, int* lanes_rows, int* lanes_cols, size_t* n_long_rows, size_t* n_long_cols, int* kp) {
    if (!o || o->kind != OBJ_SPARSE_MULTINOMIAL) return fail(QN_ERROR_INPUT_PARAMS, "not a sparse multinomial objective");
    if (nnz) *nnz = o->sm.nnz;
    if (lanes_rows) *lanes_rows = o->sm.a.lanes;
    if (lanes_cols) *lanes_cols = o->sm.at.lanes;
    if (n_long_rows) *n_long_rows = (size_t)o->sm.a.n_long;
    if (n_long_cols) *n_long_cols = (size_t)o->sm.at.n_long;
    if (kp) *kp = o->sm.kp;
    return QN_OK;
}

// the bytes one evaluation / one product moves by the model of qn_stats.obj_bytes (N = K n; each skinny matrix counted once per launch that touches it):
//   in    8 N (x) + 8 n Kp (Wt)
//   rows  12 nnz + 4 (m + 1) + 8 n Kp (Wt) + evaluation: 12 m (w, y) + 16 m Kp (C, P); product: 8 m (w) + 16 m Kp (P, T)
//   cols  12 nnz + 4 (n + 1) + 8 m Kp (C / T) + 8 n Kp (Gt)
//   out   8 n Kp (Gt) + 16 N (x, g)
static uint64_t smn_common_bytes(const qn_objective* o) {
    const uint64_t m = o->sm.m, n = (uint64_t)o->sm.nf, kp = (uint64_t)o->sm.kp;
    return 24ull * o->sm.nnz + 4ull * (m + 1) + 4ull * (n + 1) + 24ull * m * kp + 32ull * n * kp + 24ull * o->n;
}
static uint64_t smn_eval_bytes(const qn_objective* o) { return smn_common_bytes(o) + 12ull * o->sm.m; }
static uint64_t smn_product_bytes(const qn_objective* o) { return smn_common_bytes(o) + 8ull * o->sm.m; }

static QnSmnArgs smn_args(const qn_objective* o, const QnSlogCsr& c) {
    QnSmnArgs a{};
    a.row_ptr = c.row_ptr; a.col = c.col; a.val = c.val; a.wg_row_start = c.cut; a.long_rows = c.longs; a.part = c.part;
    a.G = c.G; a.n_long = c.n_long; a.K = o->sm.k; a.Kp = o->sm.kp; a.L = c.lanes; a.CL = smn_cl(o->sm.k, c.lanes); a.CLw = smn_cl(o->sm.k, 1);
    return a;
}

// the four streaming launches both modes share: xv (x or v, class-major) -> Wt, the row pass (C and P, or T from P), the column pass, and back to
// class-major with + mu xv and the shares
template <bool PRODUCT>
static int smn_enqueue_stream(qn_objective* o, const double* xv_dev, double* out_dev, double* p_dev, const QnVecCtl* ctl) {
    hipStream_t st = o->ctx->stream;
    const QnSmnTile t = smn_tile(o->sm.nf, o->sm.k, o->sm.kp);
    const int tg = smn_tile_grid(t);
    hipLaunchKernelGGL(smn_in_kernel, dim3(tg), dim3(SPQ_TPB), 0, st, t, xv_dev, (double*)o->sm.Wt, ctl, PRODUCT ? 1 : 0);
    QnSmnArgs r = smn_args(o, o->sm.a);
    r.src = o->sm.Wt; r.out = PRODUCT ? o->sm.T : o->sm.C; r.P = p_dev; r.wt = o->sm.wt; r.lab = o->sm.lab;
    smn_launch_rows<PRODUCT>(st, r, ctl);
    QnSmnArgs c = smn_args(o, o->sm.at);
    c.src = PRODUCT ? o->sm.T : o->sm.C; c.out = o->sm.Gt;
    hipLaunchKernelGGL(smn_cols_kernel, dim3(c.G + c.n_long), dim3(SPQ_TPB), 0, st, c, ctl, PRODUCT ? 1 : 0);
    hipLaunchKernelGGL(smn_out_kernel, dim3(tg), dim3(SPQ_TPB), 0, st, t, (const double*)o->sm.Gt, xv_dev, o->sm.mu, out_dev, (double*)o->sm.tpart, ctl,
                       PRODUCT ? 1 : 0);
    HIPCHK(hipGetLastError());
    return QN_OK;
}
static int smn_tile_shares(const qn_objective* o) { return smn_tile_grid(smn_tile(o->sm.nf, o->sm.k, o->sm.kp)); }

// enqueue one evaluation at x_dev (N_pad entries): f -> f_dev, g -> g_dev[0 .. N), P -> p_dev (m x Kp).  `which`: 1 the four streaming launches,
// 2 the finish, 3 all five (profiling mode times the two parts apart)
static int smn_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, double* p_dev, int which) {
    if (which & 1) QNCHK(smn_enqueue_stream<false>(o, x_dev, g_dev, p_dev, nullptr));
    if (which & 2)
        hipLaunchKernelGGL(slog_finish_kernel, dim3(1), dim3(SPQ_TPB), 0, o->ctx->stream, (const double*)o->sm.a.part, o->sm.a.G + o->sm.a.n_long,
                           (const double*)o->sm.tpart, smn_tile_shares(o), o->sm.mu, f_dev, (const QnVecCtl*)nullptr, 0);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// the same five launches at x_dev, leaving P in `sm.P` -- what the products read until the next weights pass; f and g go to scratch
static int smn_enqueue_weights(qn_objective* o, const double* x_dev) { return smn_enqueue_eval(o, x_dev, o->wp.scal, o->wp.g, o->sm.P, 3); }

// enqueue q = H v into q_dev[0 .. N) with P from `sm.P`, and v'Hv folded into wp.scal[1] (no gbar: the unnamed argument).  `ctl`: the kernels'
// predicate (NULL: unconditional).  `which`: 1 the four streaming launches, 2 the fold, 3 all five
static int smn_enqueue_hess_vec(qn_objective* o, const double* v_dev, const double*, double* q_dev, const QnVecCtl* ctl, int which) {
    if (which & 1) QNCHK(smn_enqueue_stream<true>(o, v_dev, q_dev, o->sm.P, ctl));
    if (which & 2)
        hipLaunchKernelGGL(slog_finish_kernel, dim3(1), dim3(SPQ_TPB), 0, o->ctx->stream, (const double*)nullptr, 0, (const double*)o->sm.tpart,
                           smn_tile_shares(o), o->sm.mu, (double*)o->wp.scal + 1, ctl, 1);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// P at x (m x K, row-major) for the tests and for callers that want the class probabilities: one weights pass
extern "C" int qn_sparse_multinomial_probabilities(qn_objective* o, const double* x_host, double* p_host) {
    if (!o || o->kind != OBJ_SPARSE_MULTINOMIAL || !x_host || !p_host) return fail(QN_ERROR_INPUT_PARAMS, "not a sparse multinomial objective, or a null argument");
    qn_context* c = o->ctx;
    HIPCHK(hipSetDevice(c->device));
    QNCHK(o->ex.ensure(2 * (size_t)o->T.n_pad, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(smn_enqueue_weights(o, o->ex));
    const size_t K = (size_t)o->sm.k;
    HIPCHK(hipMemcpy2DAsync(p_host, K * sizeof(double), o->sm.P, (size_t)o->sm.kp * sizeof(double), K * sizeof(double), o->sm.m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return QN_OK;
}

// the table's evaluation: P goes to the trial buffer -- `sm.P` keeps the last weights pass's P, NewtonCG's at x_k
static int smn_eval_trial(qn_objective* o, const double* x, double* f, double* g, int which, const QnObjWork*) { return smn_enqueue_eval(o, x, f, g, o->sm.P_trial, which); }
// v'Hv: one value, folded by the product's fifth launch
static int smn_hv_out(qn_objective* o, QnHvOut* out) { *out = QnHvOut{o->wp.scal + 1, 1, false}; return QN_OK; }

// kernels of its own (no limit on K n): transpose in, rows, columns, transpose out, then the fold, which is timed with the control kernels
static const QnObjOps kSmnOps = {
    /* eval */ smn_eval_trial, /* eval_launches */ 5, /* eval_split */ true, /* vec_counted */ true,
    /* weights */ smn_enqueue_weights, 5,
    /* hv_built, hess_vec, gbar, hv_out */ nullptr, smn_enqueue_hess_vec, wp_zero_gbar, smn_hv_out, 5, true,
    /* curvature, curv_shares; hessian */ nullptr, nullptr, nullptr, 0,
    /* bytes: eval, product, weights, curvature */ smn_eval_bytes, smn_product_bytes, smn_eval_bytes, nullptr,
    /* no_dense_family */ QN_VEC_FAMILY_ONLY("SparseMultinomial"),
    /* no_rows */ "a sparse multinomial objective has no dense rows / Hessian",
    /* no_hessian */ "a sparse multinomial objective has no dense rows / Hessian: hess_vec_at gives H(x) v",
    /* no_curvature */ "qn_objective_hess_vec: the Hessian of a sparse multinomial objective depends on x: use qn_objective_hess_vec_at",
};

// the device side of a new objective: both copies, the labels, the weights and every buffer the launches above use.  The staging vectors live until
// the stream is idle.
static int smn_fill(qn_objective* o, const std::vector<int>& rp, const std::vector<int>& ci, const double* val, const int* lab_host, const double* w_host) {
    const size_t n = (size_t)o->sm.nf, m = o->sm.m, nnz = o->sm.nnz, np = o->T.n_pad, kp = (size_t)o->sm.kp;
    hipStream_t st = o->ctx->stream;
    std::vector<int> tp, tc;
    std::vector<double> tv;
    qn_csr::transpose(m, n, rp.data(), ci.data(), val, tp, tc, tv);
    const qn_csr::Cut ca = qn_csr::cut(m, rp.data(), SPQ_MAXG, SPQ_LONG_ROW), cat = qn_csr::cut(n, tp.data(), SPQ_MAXG, SPQ_LONG_ROW);
    int status = slog_upload(o->sm.a, m, rp, ci, val, nnz, ca, st);
    if (status == QN_OK) status = slog_upload(o->sm.at, n, tp, tc, tv.data(), nnz, cat, st);
    o->sm.a.lanes = o->sm.a.lanes_auto = smn_auto_lanes(ca.lanes, o->sm.k);
    o->sm.at.lanes = o->sm.at.lanes_auto = smn_auto_lanes(cat.lanes, o->sm.k);
    if (status == QN_OK) status = o->sm.lab.alloc(m);
    if (status == QN_OK) status = o->sm.wt.alloc_zero(m, st);
    if (status == QN_OK) status = o->sm.Wt.alloc_zero(n * kp, st);       // x or v, feature-major
    if (status == QN_OK) status = o->sm.Gt.alloc_zero(n * kp, st);       // A'C or A'T, feature-major
    if (status == QN_OK) status = o->sm.C.alloc_zero(m * kp, st);        // the coefficients of one evaluation (its margins while the class blocks go by)
    if (status == QN_OK) status = o->sm.T.alloc_zero(m * kp, st);        // t of one product
    if (status == QN_OK) status = o->sm.P.alloc_zero(m * kp, st);        // P at the accepted point (what the products read)
    if (status == QN_OK) status = o->sm.P_trial.alloc_zero(m * kp, st);  // P of trial evaluations: never read
    if (status == QN_OK) status = o->sm.tpart.alloc_zero(SMN_TGRID, st); // the shares of ||x||^2 or v.q
    if (status == QN_OK) status = o->wp.zero.alloc_zero(np, st);         // NewtonCG's gbar slot
    if (status == QN_OK) status = o->wp.g.alloc_zero(np, st);            // g of a weights pass
    if (status == QN_OK) status = o->wp.scal.alloc_zero(2, st);          // f of a weights pass; v'Hv of a product
    if (status == QN_OK && (hipMemcpyAsync(o->sm.lab, lab_host, m * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
                            hipMemcpyAsync(o->sm.wt, w_host, m * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess))
        status = fail(QN_ABNORMAL_TERMINATION, "sparse multinomial: the upload of the labels and the weights failed");
    const hipError_t e = hipStreamSynchronize(st); // (also after a failure: the copies enqueued so far read the vectors above)
    if (status == QN_OK && e != hipSuccess) status = fail(QN_ABNORMAL_TERMINATION, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return status;
}

extern "C" int qn_sparse_multinomial_create(qn_context* ctx, size_t m, size_t n, size_t k, size_t nnz, const void* row_ptr_host, const void* col_idx_host,
                                            int index_bytes, const double* values_host, const void* labels_i32_host, const double* w_host, double mu,
                                            qn_objective** out) {
    const int32_t* labels_host = (const int32_t*)labels_i32_host;
    if (!ctx || !out || !row_ptr_host || !col_idx_host || !values_host || !labels_host || n == 0 || m == 0)
        return fail(QN_ERROR_INPUT_PARAMS, "null argument or empty shape");
    if (index_bytes != 4 && index_bytes != 8) return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: index_bytes must be 4 or 8");
    if (k < 2) return fail(QN_ERROR_INPUT_PARAMS, "the sparse multinomial objective is not built for fewer than 2 classes");
    if (n > (size_t)1 << 30 || m > (size_t)1 << 30 || k > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "shape too large");
    if (nnz > (size_t)INT32_MAX) return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: nnz must not exceed 2^31 - 1");
    if (m * k > (size_t)INT32_MAX) return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: m K must not exceed 2^31 - 1");
    if (n * k > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: K n must not exceed 2^30 (the solvers' vectors)");
    if (!std::isfinite(mu)) return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: mu must be finite");
    if (ctx->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "the sparse multinomial objective is single-GPU (it lives on one rank: no row sharding)");
    std::vector<double> w(m);
    for (size_t i = 0; i < m; ++i) { // qn_multinomial_create's rules
        if (labels_host[i] < 0 || (size_t)labels_host[i] >= k)
            return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: labels[" + std::to_string(i) + "] is outside [0, n_classes)");
        w[i] = w_host ? w_host[i] : 1.0;
        if (!(w[i] >= 0.0) || !std::isfinite(w[i]))
            return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: weights[" + std::to_string(i) + "] is negative or not finite (a weight of 0 masks its row)");
    }
    std::string err;
    const bool ok = index_bytes == 4 ? qn_csr::validate(m, n, nnz, (const int32_t*)row_ptr_host, (const int32_t*)col_idx_host, &err)
                                     : qn_csr::validate(m, n, nnz, (const int64_t*)row_ptr_host, (const int64_t*)col_idx_host, &err);
    if (!ok) return fail(QN_ERROR_INPUT_PARAMS, "sparse multinomial: " + err);
    std::vector<int> rp, ci;
    if (index_bytes == 4) qn_csr::narrow(m, nnz, (const int32_t*)row_ptr_host, (const int32_t*)col_idx_host, rp, ci);
    else qn_csr::narrow(m, nnz, (const int64_t*)row_ptr_host, (const int64_t*)col_idx_host, rp, ci);
    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    o->ctx = ctx; o->kind = OBJ_SPARSE_MULTINOMIAL; o->ops = &kSmnOps; o->n = n * k;
    o->sm.m = m; o->sm.mu = mu; o->sm.nnz = nnz; o->sm.k = (int)k; o->sm.nf = (int)n; o->sm.kp = smn_kp((int)k);
    o->T = make_tile(n * k, ctx, 1); // (the padding of the solver's vectors: N = K n entries)
    const int st = smn_fill(o, rp, ci, values_host, labels_host, w.data());
    if (st != QN_OK) { delete o; return st; } // (*out is written only for an objective that is whole: a failed creation leaks nothing)
    *out = o;
    return QN_OK;
}
