// qn_host_objective.hip.h -- host side, device-resident objectives: the state blocks of qn_objective and the operations table every kind fills
// (QnObjOps), the creation of the dense quadratic, the log-sum-exp and the sparse quadratic, the first two's evaluation launches, and the host entry
// points every kind answers through its table (qn_objective_eval, _hessian, _get_rows).  The logistic pair and the multinomial are created in
// qn_host_logistic.hip.h, qn_host_sparse_logistic.hip.h, qn_host_multinomial.hip.h and qn_host_sparse_multinomial.hip.h.
#pragma once
#include "qn_csr_host.h"
// ------------------------------------------------------------------------------------------------
// objectives
// ------------------------------------------------------------------------------------------------
enum { OBJ_QUADRATIC = 1, OBJ_LOGSUMEXP = 2, OBJ_SPARSE_QUADRATIC = 3, OBJ_LOGISTIC = 4, OBJ_SPARSE_LOGISTIC = 5, OBJ_MULTINOMIAL = 6, OBJ_SPARSE_MULTINOMIAL = 7 };
// the sparse quadratic's launch shape (qn_sparse.hip.h; the creation below cuts the rows for it)
#define SPQ_MAXG 2048     // regular workgroups at the most: 8 per CU on 256 CUs
#define SPQ_LONG_ROW 2048 // rows longer than this get a workgroup of their own
// one CSR copy of the sparse logistic objective (qn_sparse_logistic.hip.h): the matrix, its static cut, its long rows, its shares, its lanes per row
struct QnSlogCsr {
    DevBuf<int> row_ptr, col, cut, longs;
    DevBuf<double> val, part;
    size_t rows = 0;
    int G = 0, n_long = 0, lanes = 1, lanes_auto = 1;
};
// the multinomial objective's cut of its 512 threads (qn_multinomial.hip.h: mnl_plan)
struct QnMnlPlan { int tj_log2, KC, NC, R, RT, WQ; bool ok; };
// mnl_mfma_kernel's cut (mnl_mfma_plan); `ok`: that kernel is built for the shape
struct QnMnlMfmaPlan { int wk_log2, CTW; size_t lds; bool ok; };
static std::atomic<uint64_t> g_objective_serial{0}; // objectives are numbered at creation: an address can come back after a destroy, a serial cannot

// ---- state: one block per owner.  A kind reaches the common fields and the blocks its QnObjOps table (below) is written against, no others ----
// Quadratic, LogSumExp, Logistic, Multinomial: a dense row-major matrix, this rank's rows, and the vector that goes with its rows
struct QnDenseRows {
    DevBuf<double> rows; // Quadratic: Q, [rpr][n_pad]; the others: A, [mrpr][n_pad] (Multinomial: [mrpr][mn.nfp])
    DevBuf<double> rhs;  // Quadratic: b (n_pad); LogSumExp: c; Logistic: yw = y o w; Multinomial: the weights (m_pad each)
    size_t m = 0;        // rows of the matrix (Quadratic: n)
    QnTile TA{};         // their partition over the ranks (Quadratic: T)
    double mu = 0.0;
};
// Quadratic, SparseQuadratic
struct QnQuadState {
    bool symmetric = true; // Q == Q' bit for bit (checked at creation); the symmetric-storage evaluation needs it
};
// LogSumExp, Logistic, Multinomial: the kernels that keep a whole row per workgroup and stream A once
struct QnOneStream {
    int G = 0, kch = 0;          // the grid, and column chunks of 1024 per thread (LogSumExp: 0 where only the two-pass evaluation exists; Multinomial: not used)
    DevBuf<double> wgms, wgg;    // per-workgroup scalars (m, S / F) and per-workgroup G vectors
    DevBuf<double> z;            // margins: LogSumExp's two-pass z = A x; the logistic stream's, written and read inside its launch
    DevBuf<double> hv_shares;    // the product's combine kernel's shares of v'Hv (256 at the most) and their sum; allocated by the first product
};
// LogSumExp, Logistic, SparseLogistic, Multinomial: what a weights pass at x leaves for the Hessian-vector products that follow
struct QnWeightsPass {
    DevBuf<double> w;       // LogSumExp: the softmax weights p; the logistic pair: d at the accepted point (Multinomial keeps P in mn.P)
    DevBuf<double> w_trial; // d of the evaluations that are not a weights pass (trial points): written, never read
    DevBuf<double> zero;    // n_pad zeros: what the product's kernels take where log-sum-exp has gbar
    DevBuf<double> g;       // g of a weights pass (LogSumExp: the column sums' splits)
    DevBuf<double> scal;    // f of a weights pass; SparseLogistic: v'Hv of a product in [1]
};
struct QnLseState {
    int rs = 1;
    int two_pass = 0;           // diagnostics (QN_LSE_TWO_PASS=1 in the environment at creation): the round-1 two-pass evaluation
    DevBuf<double> gall, ms;    // the ranks' column sums A'w; the gathered per-rank (m, S) of the one-pass evaluation
};
// SparseQuadratic (qn_sparse.hip.h): Q in CSR -- int32 row offsets (n + 1), int32 columns and f64 values (nnz)
struct QnSpqState {
    DevBuf<int> row_ptr, col, wg_row_start, long_rows;
    DevBuf<double> val, b, part; // part: f's shares, one per workgroup of the evaluation launch
    size_t nnz = 0, n_long = 0;
    int G = 0;                     // regular workgroups; the long rows' run behind them in the same launch
    int lanes = 1, lanes_auto = 1; // lanes per row in use, and the choice made at creation from the mean row length
};
// SparseLogistic (qn_sparse_logistic.hip.h): A and A' in CSR (nnz entries each)
struct QnSlogState {
    QnSlogCsr a, at;
    DevBuf<double> yw, coef, t; // m each: y o w; -(yw s) of one evaluation, d o (A v) of one product -- what the column pass gathers
    size_t m = 0, nnz = 0;
    double mu = 0.0;
};
// Multinomial (qn_multinomial.hip.h): dn.rows is [mrpr][nfp], n = K n_features (class-major), T its padding
struct QnMnlState {
    int k = 0, nf = 0, nfp = 0;
    QnMnlPlan plan{};
    QnMnlMfmaPlan mfma{};
    int kernel = 1; // the stream's kernel in use: 1 mnl_onepass_kernel (vector unit), 2 mnl_mfma_kernel (qn_multinomial_set_kernel)
    DevBuf<int> lab;
    DevBuf<double> P, P_trial; // P (m_pad x K) at the accepted point, and of trial evaluations (written, never read)
};
// SparseMultinomial (qn_sparse_multinomial.hip.h): A and A' in CSR, n = K nf (class-major), T its padding; the skinny matrices have the leading dimension kp
struct QnSmnState {
    QnSlogCsr a, at;              // (`lanes`: the entry lanes L of the pass over that copy; at.part is not used)
    DevBuf<int> lab;              // m labels
    DevBuf<double> wt;            // m sample weights
    DevBuf<double> Wt, Gt;        // nf x kp: x or v feature-major; A'C or A'T before it goes back to class-major
    DevBuf<double> C, T;          // m x kp: the coefficients of one evaluation, t of one product -- what the column pass gathers
    DevBuf<double> P, P_trial;    // m x kp: P at the accepted point, and of trial evaluations (written, never read)
    DevBuf<double> tpart;         // the shares of ||x||^2 or v.q (smn_out_kernel)
    size_t m = 0, nnz = 0;
    int k = 0, nf = 0, kp = 0;
    double mu = 0.0;
};

struct QnObjOps;
struct qn_objective {
    uint64_t serial = ++g_objective_serial;
    qn_context* ctx = nullptr;
    int kind = 0;
    const QnObjOps* ops = nullptr; // the kind's launches, byte models and capabilities
    size_t n = 0;
    QnTile T{};
    DevBuf<double> ex, eq, eg, ef; // scratch of the host entry points (qn_objective_eval, _hess_vec, _hess_vec_at)
    DevBuf<double> eh; // qn_objective_hessian: the n_pad x n_pad matrix on the device (allocated by the first call)
    QnDenseRows dn;
    QnQuadState quad;
    QnOneStream os;
    QnWeightsPass wp;
    QnLseState lse;
    QnSpqState sp;
    QnSlogState sl;
    QnMnlState mn;
    QnSmnState sm;
};

// ---- operations: one table per kind, defined next to the kind's launches and set at creation ----
struct QnVecCtl;
// the two vectors the dense quadratic's row kernel wants beside the objective: its product and row-block 0's copy of the point.  NULL: the
// objective's own scratch (the host entry points, where the finish kernel reads the copy and the product is gathered over the ranks)
struct QnObjWork { double* q; double* xcopy; };
// where a product leaves v'Hv: `count` shares (their sum, by lse_hv_shares_kernel, in shares[256]) or, sum == false, the value itself
struct QnHvOut { const double* shares; int count; bool sum; };
struct QnObjOps {
    // one evaluation at x_dev: f -> f_dev, g -> g_dev; the by-product (d or P) goes to the kind's trial buffer.  `which`: 1 the streaming launches,
    // 2 the finish, 3 both.  eval_launches: what it adds to qn_stats.launches; eval_split: the first-order family times the halves apart as KC_EVAL
    // and KC_CTL (false: one KC_EVAL scope); vec_counted false: that family adds neither its launches nor its bytes (log-sum-exp, as it never has)
    int (*eval)(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, int which, const QnObjWork* w);
    int eval_launches; bool eval_split, vec_counted;
    // the weights at x for any number of products (NULL: no x-dependent Hessian-vector product), and its launches
    int (*weights)(qn_objective* o, const double* x_dev); int weights_launches;
    // q = H(x) v with the weights of the last pass: hv_built (NULL: always) refuses the shapes it does not exist for, gbar is the buffer the host
    // entry passes as gbar_dev (NewtonCG passes its copy), hv_out says where v'Hv lands.  hv_launches per product; hv_fold_ctl: the second half is
    // timed as KC_CTL (false: both halves KC_NEWTON)
    int (*hv_built)(const qn_objective* o);
    int (*hess_vec)(qn_objective* o, const double* v_dev, const double* gbar_dev, double* q_dev, const QnVecCtl* ctl, int which);
    const double* (*gbar)(const qn_objective* o);
    int (*hv_out)(qn_objective* o, QnHvOut* out);
    int hv_launches; bool hv_fold_ctl;
    // a constant Hessian: q = Q d -> q_dev and the shares of d'Qd (which & 1), d'Qd -> c_dev (which & 2).  curv_shares (NULL: none) hands the
    // shares to a caller that adds them itself (exact_step_kernel) and skips the second launch
    int (*curvature)(qn_objective* o, const double* d_dev, double* c_dev, double* q_dev, const QnVecCtl* ctl, int which, const QnObjWork* w);
    void (*curv_shares)(const qn_objective* o, const double** part, int* count);
    // the Hessian at x_dev into h_dev (leading dimension ld) and its launches; NULL with a dense Hessian: dn.rows is the Hessian
    int (*hessian)(qn_objective* o, const double* x_dev, double* h_dev, size_t ld); int hessian_launches;
    // the bytes one evaluation, product, weights pass and curvature pass move, by the model of qn_stats.obj_bytes (NULL where the pass is)
    uint64_t (*eval_bytes)(const qn_objective* o), (*hv_bytes)(const qn_objective* o), (*weights_bytes)(const qn_objective* o), (*curv_bytes)(const qn_objective* o);
    // capabilities, NULL where the kind has it, otherwise the refusal: the dense quasi-Newton family with the control-step solvers and Newton;
    // qn_objective_get_rows; a dense Hessian (the projected Newton pair wants `hessian` NULL as well: a device quadratic); qn_objective_hess_vec
    const char *no_dense_family, *no_rows, *no_hessian, *no_curvature;
    // M_j = H(x)_jj -> m_dev with the weights of the last pass, and rule 2''s 1 / M (qn_newton_cg.hip.h) -> minv_dev where that is not NULL: n_pad
    // entries each, unpredicated.  NULL: the kind has no diagonal, and every caller refuses before anything is launched.  Its launches and the
    // bytes it moves, as the members above count them
    int (*hess_diag)(qn_objective* o, double* m_dev, double* minv_dev); int diag_launches;
    uint64_t (*diag_bytes)(const qn_objective* o);
};
// the dense kinds' diagonal (qn_hess_diag.hip.h), named by the tables of LogSumExp and Logistic
static int dense_enqueue_hess_diag(qn_objective* o, double* m_dev, double* minv_dev);
#define QN_VEC_FAMILY_ONLY(name) "a " name " objective runs under SPG, projected gradient, LBFGS / ProjectedLBFGS, NonlinearCG and NewtonCG (the dense quasi-Newton family, the control-step solvers and Newton: out of scope)"
// the tables of the kinds created in this file live where all their launches are visible: qn_vec_exact.hip.h, qn_lse_hv.hip.h, qn_sparse.hip.h
static const QnObjOps* quad_ops();
static const QnObjOps* lse_ops();
static const QnObjOps* spq_ops();

static int objective_base(qn_context* ctx, size_t n, const double* b_host, qn_objective** out) {
    if (!ctx || !out || !b_host || n == 0) return fail(QN_ERROR_INPUT_PARAMS, "null argument or n == 0");
    if (n > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "n too large");
    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    o->ctx = ctx;
    o->kind = OBJ_QUADRATIC; o->ops = quad_ops();
    o->n = n;
    o->T = make_tile(n, ctx, 1);
    o->dn.m = n; o->dn.TA = o->T; // (the rows of Q are the rows qn_objective_get_rows hands out)
    *out = o;
    QNCHK(o->dn.rows.alloc_zero((size_t)o->T.rpr * o->T.n_pad, ctx->stream));
    QNCHK(o->dn.rhs.alloc_zero(o->T.n_pad, ctx->stream));
    HIPCHK(hipMemcpyAsync(o->dn.rhs, b_host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return QN_OK;
}

extern "C" int qn_quadratic_create(qn_context* ctx, size_t n, const double* q_host, const double* b_host, qn_objective** out) {
    if (!q_host) return fail(QN_ERROR_INPUT_PARAMS, "q is null");
    QNCHK(objective_base(ctx, n, b_host, out));
    qn_objective* o = *out;
    const size_t r0 = (size_t)o->T.row_off;
    if (r0 < n) {
        const size_t nr = std::min((size_t)o->T.rpr, n - r0);
        HIPCHK(hipMemcpy2D(o->dn.rows, (size_t)o->T.n_pad * sizeof(double), q_host + r0 * n, n * sizeof(double), n * sizeof(double), nr,
                           hipMemcpyHostToDevice));
    }
    // g = Q x - b is the gradient of f only for a symmetric Q, but nothing stops a caller from passing another matrix: the row
    // kernels multiply by what was given, so the symmetric-storage evaluation is used only when Q is symmetric bit for bit
    for (size_t i = 0; i < n && o->quad.symmetric; ++i)
        for (size_t j = i + 1; j < n; ++j)
            if (q_host[i * n + j] != q_host[j * n + i]) { o->quad.symmetric = false; break; }
    return QN_OK;
}

extern "C" int qn_quadratic_create_synthetic(qn_context* ctx, size_t n, uint64_t seed, const double* diag_host,
                                             const double* b_host, qn_objective** out) {
    if (!diag_host) return fail(QN_ERROR_INPUT_PARAMS, "diag is null");
    QNCHK(objective_base(ctx, n, b_host, out));
    qn_objective* o = *out;
    DevBuf<double> diag;
    QNCHK(diag.alloc(n));
    HIPCHK(hipMemcpyAsync(diag, diag_host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(synth_fill_kernel, dim3(2048), dim3(256), 0, ctx->stream, o->dn.rows, o->T, seed, diag, 1.0 / (double)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return QN_OK;
}

extern "C" int qn_logsumexp_create(qn_context* ctx, size_t m, size_t n, const double* a_host, const double* c_host, double mu,
                                   qn_objective** out) {
    if (!ctx || !out || !a_host || !c_host || n == 0 || m == 0) return fail(QN_ERROR_INPUT_PARAMS, "null argument or empty shape");
    if (n > (size_t)1 << 30 || m > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "shape too large");
    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    *out = o;
    o->ctx = ctx; o->kind = OBJ_LOGSUMEXP; o->ops = lse_ops(); o->n = n; o->dn.m = m; o->dn.mu = mu;
    o->T = make_tile(n, ctx, 1);  // column padding follows the solver's vectors
    o->dn.TA = make_tile(m, ctx, 1); // rows of A are sharded
    const size_t np = o->T.n_pad, mp = o->dn.TA.n_pad, mrpr = o->dn.TA.rpr;
    hipStream_t st = ctx->stream;
    QNCHK(o->dn.rows.alloc_zero(mrpr * np, st));
    QNCHK(o->dn.rhs.alloc_zero(mp, st));
    HIPCHK(hipMemcpyAsync(o->dn.rhs, c_host, m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // the zero-fill above must land before the (null-stream) 2-D upload below
    const size_t r0 = (size_t)o->dn.TA.row_off;
    if (r0 < m) {
        const size_t nr = std::min(mrpr, m - r0);
        HIPCHK(hipMemcpy2D(o->dn.rows, np * sizeof(double), a_host + r0 * n, n * sizeof(double), n * sizeof(double), nr, hipMemcpyHostToDevice));
    }
    o->lse.rs = (int)std::max<size_t>(1, std::min<size_t>(64, mrpr / 64));
    QNCHK(o->os.z.alloc_zero((size_t)ctx->world * 2 * mrpr, st));
    QNCHK(o->wp.w.alloc_zero(mp, st));
    QNCHK(o->wp.g.alloc_zero((size_t)o->lse.rs * np, st));
    QNCHK(o->lse.gall.alloc_zero((size_t)ctx->world * np, st));
    QNCHK(o->wp.scal.alloc_zero(2, st));
    o->lse.two_pass = getenv("QN_LSE_TWO_PASS") && atoi(getenv("QN_LSE_TWO_PASS")) != 0;
    if (np <= 16384 && np >= 2) { // the one-pass evaluation keeps a whole row per workgroup in registers
        int kch = 1;
        while ((size_t)kch * 1024 < np) kch *= 2;
        o->os.kch = kch;
        o->os.G = (int)std::max<size_t>(1, std::min<size_t>(256, (mrpr + 3) / 4));
        QNCHK(o->os.wgms.alloc_zero(2 * (size_t)o->os.G, st));
        QNCHK(o->os.wgg.alloc_zero((size_t)o->os.G * np, st));
        QNCHK(o->lse.ms.alloc_zero(2 * (size_t)ctx->world, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return QN_OK;
}

// ---- the sparse quadratic: f = 1/2 x'Qx - b'x with Q in CSR (kernels, launches and its table: qn_sparse.hip.h) ----
template <class I>
static int spq_validate(size_t n, size_t nnz, const I* rp, const I* ci) {
    if (rp[0] != 0) return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: row_ptr[0] must be 0");
    if (rp[n] < 0 || (uint64_t)rp[n] != (uint64_t)nnz) return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: row_ptr[n] must be nnz");
    for (size_t i = 0; i < n; ++i) {
        if (rp[i + 1] < rp[i]) return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: row_ptr decreases at row " + std::to_string(i));
        if ((uint64_t)rp[i + 1] > (uint64_t)nnz) return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: row_ptr exceeds nnz at row " + std::to_string(i));
        for (size_t j = (size_t)rp[i]; j < (size_t)rp[i + 1]; ++j) {
            if (ci[j] < 0 || (uint64_t)ci[j] >= (uint64_t)n)
                return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: a column of row " + std::to_string(i) + " is outside [0, n)");
            if (j > (size_t)rp[i] && ci[j] <= ci[j - 1])
                return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: the columns of row " + std::to_string(i) + " are not strictly increasing (unsorted or duplicate)");
        }
    }
    return QN_OK;
}

extern "C" int qn_sparse_quadratic_create(qn_context* ctx, size_t n, size_t nnz, const void* row_ptr_host, const void* col_idx_host,
                                          int index_bytes, const double* values_host, const double* b_host, qn_objective** out) {
    if (!ctx || !out || !row_ptr_host || !col_idx_host || !values_host || !b_host || n == 0)
        return fail(QN_ERROR_INPUT_PARAMS, "null argument or n == 0");
    if (index_bytes != 4 && index_bytes != 8) return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: index_bytes must be 4 or 8");
    if (n > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "n too large");
    if (nnz > (size_t)INT32_MAX) return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: nnz must not exceed 2^31 - 1");
    if (ctx->world > 1) return fail(QN_ERROR_INPUT_PARAMS, "a sparse quadratic lives on one rank (no row sharding)");
    if (index_bytes == 4) QNCHK(spq_validate(n, nnz, (const int32_t*)row_ptr_host, (const int32_t*)col_idx_host));
    else QNCHK(spq_validate(n, nnz, (const int64_t*)row_ptr_host, (const int64_t*)col_idx_host));
    // the device's copy (int32 whatever came in), symmetry bit for bit -- the transpose's rows come out with increasing columns: compared with what
    // was given --, and the static cut of the rows over workgroups with the lanes per row (qn_csr_host.h: the sparse logistic objective's rules).
    // Lanes, measured (tools/bench_sparse.py): the five-point Laplacian (5 per row) is fastest with 2 lanes, a random pattern of 17
    // per row with 16 to 32 (8 lanes: 9 % behind)
    std::vector<int> rp, ci, tp, tc;
    std::vector<double> tv;
    if (index_bytes == 4) qn_csr::narrow(n, nnz, (const int32_t*)row_ptr_host, (const int32_t*)col_idx_host, rp, ci);
    else qn_csr::narrow(n, nnz, (const int64_t*)row_ptr_host, (const int64_t*)col_idx_host, rp, ci);
    qn_csr::transpose(n, n, rp.data(), ci.data(), values_host, tp, tc, tv);
    const bool symmetric = tp == rp && memcmp(tc.data(), ci.data(), nnz * sizeof(int)) == 0 && memcmp(tv.data(), values_host, nnz * sizeof(double)) == 0;
    const qn_csr::Cut cut = qn_csr::cut(n, rp.data(), SPQ_MAXG, SPQ_LONG_ROW);
    const std::vector<int>& longs = cut.longs;
    const int G = cut.G;

    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    *out = o;
    o->ctx = ctx; o->kind = OBJ_SPARSE_QUADRATIC; o->ops = spq_ops(); o->n = n;
    o->T = make_tile(n, ctx, 1); // (the padding of the solver's vectors)
    o->quad.symmetric = symmetric;
    o->sp.nnz = nnz; o->sp.n_long = longs.size(); o->sp.G = G;
    o->sp.lanes = o->sp.lanes_auto = cut.lanes;
    hipStream_t st = ctx->stream;
    QNCHK(o->sp.b.alloc_zero(o->T.n_pad, st));
    QNCHK(o->sp.row_ptr.alloc(n + 1));
    QNCHK(o->sp.col.alloc(std::max<size_t>(nnz, 1)));
    QNCHK(o->sp.val.alloc_zero(std::max<size_t>(nnz, 1), st));
    QNCHK(o->sp.wg_row_start.alloc((size_t)G + 1));
    QNCHK(o->sp.long_rows.alloc(std::max<size_t>(longs.size(), 1)));
    QNCHK(o->sp.part.alloc_zero((size_t)G + longs.size(), st));
    HIPCHK(hipMemcpyAsync(o->sp.b, b_host, n * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->sp.row_ptr, rp.data(), (n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->sp.col, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (nnz) HIPCHK(hipMemcpyAsync(o->sp.val, values_host, nnz * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->sp.wg_row_start, cut.start.data(), cut.start.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!longs.empty()) HIPCHK(hipMemcpyAsync(o->sp.long_rows, longs.data(), longs.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // (the staging vectors above go out of scope)
    return QN_OK;
}

extern "C" int qn_sparse_quadratic_set_lanes_per_row(qn_objective* o, int lanes) {
    if (!o || o->kind != OBJ_SPARSE_QUADRATIC) return fail(QN_ERROR_INPUT_PARAMS, "lanes_per_row belongs to a sparse quadratic");
    if (lanes == 0) { o->sp.lanes = o->sp.lanes_auto; return QN_OK; }
    if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1)) != 0)
        return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: lanes_per_row must be 0 (automatic), 1, 2, 4, 8, 16, 32 or 64");
    o->sp.lanes = lanes;
    return QN_OK;
}

extern "C" int qn_objective_sparse_info(qn_objective* o, size_t* nnz, int* lanes_per_row, size_t* n_long_rows, int* symmetric) {
    if (o && o->kind == OBJ_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "a logistic objective is not a sparse quadratic (its A is dense)");
    if (o && o->kind == OBJ_SPARSE_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "a sparse logistic objective is not a sparse quadratic: qn_sparse_logistic_info describes it");
    if (o && o->kind == OBJ_MULTINOMIAL) return fail(QN_ERROR_INPUT_PARAMS, "a multinomial objective is not a sparse quadratic (its A is dense)");
    if (o && o->kind == OBJ_SPARSE_MULTINOMIAL) return fail(QN_ERROR_INPUT_PARAMS, "a sparse multinomial objective is not a sparse quadratic: qn_sparse_multinomial_info describes it");
    if (!o || o->kind != OBJ_SPARSE_QUADRATIC) return fail(QN_ERROR_INPUT_PARAMS, "not a sparse quadratic");
    if (nnz) *nnz = o->sp.nnz;
    if (lanes_per_row) *lanes_per_row = o->sp.lanes;
    if (n_long_rows) *n_long_rows = o->sp.n_long;
    if (symmetric) *symmetric = o->quad.symmetric ? 1 : 0;
    return QN_OK;
}

template <int R>
static void launch_hpass(hipStream_t st, const QnHPassArgs& a);

// the one-pass kernels (evaluation, product, the logistic stream) are built for 1, 2, 4, 8 and 16 column chunks of 1024 per thread: calls
// f(std::integral_constant<int, KCH>{}) for the objective's count
template <class F>
static int lse_kch_call(int kch, F&& f) {
    switch (kch) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
    }
}

// enqueue one evaluation of the log-sum-exp objective at x_dev (n_pad entries): f -> f_dev, g -> g_dev
template <int KCH, bool NTA>
static int lse_launch_onepass_nt(hipStream_t st, int G, const QnLseArgs& a, double* wgms, double* wgg) {
    static std::atomic<bool> attr_set[64]; // per device: hipFuncSetAttribute applies to the current device only (atomic: ranks may be threads)
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t lds = (size_t)KCH * 1024 * sizeof(double);
    if ((dev < 0 || dev >= 64 || !attr_set[dev].load()) && lds > 48 * 1024) { // x in LDS: up to 128 KB of the CU's 160 KB
        if (hipFuncSetAttribute((const void*)lse_onepass_kernel<KCH, NTA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return -1; // this device does not grant the LDS: the caller keeps the two-pass evaluation
        }
        if (dev >= 0 && dev < 64) attr_set[dev].store(true);
    }
    hipLaunchKernelGGL((lse_onepass_kernel<KCH, NTA>), dim3(G), dim3(512), lds, st, a, wgms, wgg);
    return QN_OK;
}
template <int KCH>
static int lse_launch_onepass(hipStream_t st, int G, const QnLseArgs& a, double* wgms, double* wgg) {
    // rows of A that cannot stay in the 256 MB Infinity Cache between evaluations are requested as non-temporal (QN_LSE_NT = 0 / 1 overrides)
    static const int nt_env = getenv("QN_LSE_NT") ? atoi(getenv("QN_LSE_NT")) : -1;
    const bool nt = nt_env >= 0 ? nt_env != 0 : (size_t)a.mrpr * (size_t)a.n_pad * sizeof(double) > ((size_t)230 << 20);
    return nt ? lse_launch_onepass_nt<KCH, true>(st, G, a, wgms, wgg) : lse_launch_onepass_nt<KCH, false>(st, G, a, wgms, wgg);
}

// the first launches of the two-pass evaluation at x_dev: z = A_rows x, the softmax weights NORMALISED into `wp.w` (zero past row m), this rank's
// column sums A'w into its block of `lse.gall`, f's terms into `wp.scal` -- what lse_finish_kernel needs, and what the Hessian needs (p and gbar)
static int lse_enqueue_weights(qn_objective* o, const double* x_dev, QnLseArgs& a) {
    qn_context* c = o->ctx;
    hipStream_t st = c->stream;
    // pass 1: z = A_rows x (the H-pass kernel in plain mat-vec mode)
    QnHPassArgs h{};
    h.H = o->dn.rows; h.T = o->dn.TA; h.T.n_pad = o->T.n_pad; h.T.n = (int)o->n; h.T.cs = 1;
    h.T.rpr = o->dn.TA.rpr; h.T.row_off = 0; // row guards are not needed for a read-only pass
    h.hp = o->os.z; h.expect_phase = -1; h.force_nrhs = 1; h.force_pending = 0; h.r0 = x_dev; h.r1 = x_dev;
    h.sp = x_dev; h.up = x_dev;
    launch_hpass<8>(st, h);
    HIPCHK(hipGetLastError());
    c->n_xchg_vector++;
    QNCHK(exchange(c, o->os.z, 2 * (size_t)o->dn.TA.rpr));
    a = QnLseArgs{};
    a.A = o->dn.rows; a.c = o->dn.rhs; a.z = o->os.z; a.w = o->wp.w; a.gpart = o->wp.g; a.gall = o->lse.gall; a.x = x_dev;
    a.scal = o->wp.scal; a.mu = o->dn.mu;
    a.m = (int)o->dn.m; a.m_pad = o->dn.TA.n_pad; a.mrpr = o->dn.TA.rpr; a.n = (int)o->n; a.n_pad = o->T.n_pad;
    a.world = c->world; a.rank = c->rank; a.rs = o->lse.rs;
    hipLaunchKernelGGL(lse_softmax_kernel, dim3(1), dim3(1024), 0, st, a);
    // pass 2: column sums A'w over this rank's rows
    hipLaunchKernelGGL(lse_colsum_kernel, dim3((a.n_pad + QN_CHUNK - 1) / QN_CHUNK, a.rs), dim3(QN_TPB), 0, st, a);
    hipLaunchKernelGGL(lse_reduce_splits_kernel, dim3(std::min(1024, (a.n_pad + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// (`which` and the work vectors are the table's signature: one KC_EVAL scope, no work vectors)
static int lse_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, int = 3, const QnObjWork* = nullptr) {
    qn_context* c = o->ctx;
    hipStream_t st = c->stream;
    if (o->os.kch && !o->lse.two_pass) { // one pass over A (qn_kernels.hip.h): 8 m n / P bytes per evaluation instead of 16 m n / P
        QnLseArgs a{};
        a.A = o->dn.rows; a.c = o->dn.rhs; a.gall = o->lse.gall; a.x = x_dev; a.f_out = f_dev; a.g_out = g_dev; a.mu = o->dn.mu;
        a.m = (int)o->dn.m; a.m_pad = o->dn.TA.n_pad; a.mrpr = o->dn.TA.rpr; a.n = (int)o->n; a.n_pad = o->T.n_pad;
        a.world = c->world; a.rank = c->rank; a.rs = 1;
        const int lst = lse_kch_call(o->os.kch, [&](auto K) { return lse_launch_onepass<decltype(K)::value>(st, o->os.G, a, o->os.wgms, o->os.wgg); });
        if (lst < 0) { o->lse.two_pass = 1; return lse_enqueue_eval(o, x_dev, f_dev, g_dev); }
        hipLaunchKernelGGL(lse_combine_kernel, dim3((a.n_pad + 63) / 64), dim3(256), 0, st, a, o->os.G, o->os.wgms, o->os.wgg, o->lse.ms);
        HIPCHK(hipGetLastError());
        const XchgItem items[2] = {{o->lse.gall, (size_t)a.n_pad}, {o->lse.ms, 2}};
        c->n_xchg_vector++;
        QNCHK(exchange_group(c, items, 2));
        hipLaunchKernelGGL(lse_finish1_kernel, dim3(std::min(1024, (a.n_pad + 255) / 256)), dim3(256), 0, st, a, o->lse.ms);
        HIPCHK(hipGetLastError());
        return QN_OK;
    }
    QnLseArgs a{};
    QNCHK(lse_enqueue_weights(o, x_dev, a));
    a.f_out = f_dev; a.g_out = g_dev;
    c->n_xchg_vector++;
    QNCHK(exchange(c, o->lse.gall, (size_t)a.n_pad));
    hipLaunchKernelGGL(lse_finish_kernel, dim3(std::min(1024, (a.n_pad + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// enqueue the Hessian of the log-sum-exp objective at x_dev (n_pad entries) into h_dev: n_pad x n_pad, row-major with leading dimension ld,
// H == H' bit for bit (qn_lse_hess.hip.h).  One rank; everything on the context's stream, no host synchronisation.
static int lse_hess_launch(hipStream_t st, const double* A, const double* p, const double* gbar, double mu, int m, int np, double* H, size_t ld);
static int lse_enqueue_hessian(qn_objective* o, const double* x_dev, double* h_dev, size_t ld) {
    if (o->ctx->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "the log-sum-exp Hessian is single-GPU");
    QnLseArgs a{};
    QNCHK(lse_enqueue_weights(o, x_dev, a)); // p -> wp.w, gbar -> lse.gall (rank 0's block is the whole sum on one rank)
    return lse_hess_launch(o->ctx->stream, o->dn.rows, o->wp.w, o->lse.gall, o->dn.mu, (int)o->dn.m, o->T.n_pad, h_dev, ld);
}

extern "C" void qn_objective_destroy(qn_objective* o) {
    if (!o) return;
    (void)hipSetDevice(o->ctx->device);
    delete o;
}

extern "C" int qn_objective_get_rows(qn_objective* o, size_t row0, size_t nrows, double* out_host) {
    if (o->ops->no_rows) return fail(QN_ERROR_INPUT_PARAMS, o->ops->no_rows);
    const size_t lo = (size_t)o->dn.TA.row_off, hi = std::min(o->dn.m, lo + (size_t)o->dn.TA.rpr); // (Q's rows, or the dense A's)
    if (row0 < lo || row0 + nrows > hi) return fail(QN_ERROR_INPUT_PARAMS, "rows outside this rank's shard");
    HIPCHK(hipSetDevice(o->ctx->device));
    HIPCHK(hipMemcpy2D(out_host, o->n * sizeof(double), o->dn.rows + (row0 - lo) * (size_t)o->T.n_pad, (size_t)o->T.n_pad * sizeof(double),
                       o->n * sizeof(double), nrows, hipMemcpyDeviceToHost));
    return QN_OK;
}

template <int R>
static void launch_quad(hipStream_t st, const QnQuadArgs& a) {
    dim3 grid(a.T.rpr / R, a.T.cs);
    hipLaunchKernelGGL(quad_matvec_kernel<R>, grid, dim3(QN_TPB), 0, st, a);
}
static int launch_quad_R(int R, hipStream_t st, const QnQuadArgs& a) {
    switch (R) {
    case 4: launch_quad<4>(st, a); break;
    case 16: launch_quad<16>(st, a); break;
    default: launch_quad<8>(st, a); break;
    }
    HIPCHK(hipGetLastError());
    return QN_OK;
}

__global__ __launch_bounds__(QN_CTL_TPB) void quad_finish_kernel(const QnVecs V, double* f_out, double* g_out) {
    __shared__ double lds[32];
    double p[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < V.n_pad; i += QN_CTL_TPB) {
        const double qi = q_val(V, i), xi = V.xt[i], bi = V.b[i];
        p[0] = __builtin_fma(xi, qi, p[0]);
        p[1] = __builtin_fma(bi, xi, p[1]);
        g_out[i] = qi - bi;
    }
    ctl_block_sum<2>(p, lds);
    if (threadIdx.x == 0) *f_out = 0.5 * p[0] - p[1];
}

// the dense quadratic's two passes over v_dev share these: the work vectors (`w`, or the objective's own scratch where the host entry points upload
// v to o->ex), and what the finish kernels read -- the product and the point (the caller's, or row-block 0's copy of it)
static int quad_vecs(qn_objective* o, const double* v_dev, const QnObjWork* w, QnVecs* V, double** xcopy) {
    const size_t np = o->T.n_pad;
    if (!w) QNCHK(o->eq.ensure(np, o->ctx->stream));
    *xcopy = w ? w->xcopy : o->ex + np;
    V->q = w ? w->q : (double*)o->eq;
    V->xt = w ? (double*)v_dev : *xcopy;
    V->n = (int)o->n; V->n_pad = (int)np; V->rpr = o->T.rpr; V->world = o->ctx->world; V->qcs = 1; V->hcs = 1;
    return QN_OK;
}
// this rank's rows of Q v by the row kernel
static int quad_enqueue_rows(qn_objective* o, const double* v_dev, const QnVecs& V, double* xcopy) {
    QnQuadArgs a{};
    a.Q = o->dn.rows; a.T = o->T; a.x = v_dev; a.d = v_dev; a.xt = xcopy;
    a.out = V.q + (size_t)o->ctx->rank * o->T.rpr;
    a.ctl = nullptr; a.expect_phase = -1; a.force_kind = QN_REQ_X; a.force_t = 0.0;
    return launch_quad_R(8, o->ctx->stream, a);
}

// enqueue one evaluation of the dense quadratic at x_dev: Q x by the row kernel (gathered over the ranks), then f and g = Q x - b
static int quad_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, int, const QnObjWork* w) {
    qn_context* c = o->ctx;
    QnVecs V{};
    double* xcopy = nullptr;
    QNCHK(quad_vecs(o, x_dev, w, &V, &xcopy));
    QNCHK(quad_enqueue_rows(o, x_dev, V, xcopy));
    QNCHK(exchange(c, V.q, (size_t)o->T.rpr));
    V.b = o->dn.rhs;
    hipLaunchKernelGGL(quad_finish_kernel, dim3(1), dim3(QN_CTL_TPB), 0, c->stream, V, f_dev, g_dev);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

extern "C" int qn_objective_eval(qn_objective* o, const double* x_host, double* f, double* g_host) {
    qn_context* c = o->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t np = o->T.n_pad;
    QNCHK(o->ex.ensure(2 * np, c->stream)); // x, and the dense quadratic's copy of it
    QNCHK(o->eg.ensure(np, c->stream));
    QNCHK(o->ef.ensure(2, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(o->ops->eval(o, o->ex, o->ef, o->eg, 3, nullptr)); // (the by-product goes to the trial buffer: the last weights pass's d or P stays)
    HIPCHK(hipMemcpyAsync(f, o->ef, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(g_host, o->eg, o->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return QN_OK;
}

extern "C" int qn_objective_hessian(qn_objective* o, const double* x_host, double* h_colmajor_host) {
    if (!o || !x_host) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (o->ops->no_hessian) return fail(QN_ERROR_INPUT_PARAMS, o->ops->no_hessian);
    qn_context* c = o->ctx;
    if (c->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "qn_objective_hessian is single-GPU");
    HIPCHK(hipSetDevice(c->device));
    const size_t n = o->n, np = o->T.n_pad;
    if (!o->ops->hessian) { // a quadratic: Q itself, whatever x is
        if (!h_colmajor_host) return QN_OK;
        std::vector<double> rows(n * n);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy2D(rows.data(), n * sizeof(double), o->dn.rows, np * sizeof(double), n * sizeof(double), n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < n; ++j) h_colmajor_host[i + j * n] = rows[i * n + j];
        return QN_OK;
    }
    QNCHK(o->ex.ensure(2 * np, c->stream));
    QNCHK(o->eh.ensure(np * np));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(o->ops->hessian(o, o->ex, o->eh, np));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!h_colmajor_host) return QN_OK; // (the launches alone: what tools/bench_lse_hessian.py times)
    // H == H' bit for bit: its rows are its columns
    HIPCHK(hipMemcpy2D(h_colmajor_host, n * sizeof(double), o->eh, np * sizeof(double), n * sizeof(double), n, hipMemcpyDeviceToHost));
    return QN_OK;
}
