// qn_host_objective.hip.h -- host side, part 3 of 7: device-resident objectives (the synthetic quadratic, the log-sum-exp, the sparse quadratic, the logistic pair, the multinomial) and their evaluation launches.
#pragma once
// ------------------------------------------------------------------------------------------------
// objectives
// ------------------------------------------------------------------------------------------------
enum { OBJ_QUADRATIC = 1, OBJ_LOGSUMEXP = 2, OBJ_SPARSE_QUADRATIC = 3, OBJ_LOGISTIC = 4, OBJ_SPARSE_LOGISTIC = 5, OBJ_MULTINOMIAL = 6 };
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
struct qn_objective {
    uint64_t serial = ++g_objective_serial;
    qn_context* ctx = nullptr;
    int kind = 0;
    size_t n = 0;
    QnTile T{};
    DevBuf<double> Q; // this rank's rows, [rpr][n_pad]
    DevBuf<double> b; // n_pad
    bool q_symmetric = true; // quadratic: Q == Q' bit for bit (checked at creation); the symmetric-storage evaluation needs it
    // scratch for qn_objective_eval
    DevBuf<double> ex, eq, eg, ef;
    DevBuf<double> eh; // qn_objective_hessian: the n_pad x n_pad matrix on the device (allocated by the first call)
    // log-sum-exp: A rows are in Q ([mrpr][n_pad]), c in b (m_pad)
    size_t m = 0;
    QnTile TA{}; // row partition of A (m rows)
    double mu = 0.0;
    int lse_rs = 1;
    int lse_two_pass = 0; // diagnostics (QN_LSE_TWO_PASS=1 in the environment at creation): the round-1 two-pass evaluation
    DevBuf<double> lz, lw, lgpart, lgall, lscal;
    DevBuf<double> lwgms, lwgg, lms; // one-pass evaluation: per-workgroup (m, S), G vectors; gathered per-rank (m, S)
    int lse_G = 0, lse_kch = 0;                                 // its grid and column chunks per thread (0: two-pass evaluation)
    DevBuf<double> lhv_shares; // qn_lse_hv.hip.h: the combine kernel's shares of v'Hv (256 at the most) and their sum; allocated by the first product
    // sparse quadratic (qn_sparse.hip.h): Q in CSR -- int32 row offsets (n + 1), int32 columns and f64 values (nnz) --, b in `b`
    DevBuf<int> sp_row_ptr, sp_col, sp_wg_row_start, sp_long_rows;
    DevBuf<double> sp_val, sp_part; // sp_part: f's shares, one per workgroup of the evaluation launch
    size_t sp_nnz = 0, sp_n_long = 0;
    int sp_G = 0;                    // regular workgroups; the long rows' run behind them in the same launch
    int sp_lanes = 1, sp_lanes_auto = 1; // lanes per row in use, and the choice made at creation from the mean row length
    // logistic (qn_logistic.hip.h): A rows in Q, yw = y o w in b (m_pad); lse_G / lse_kch, lwgms (the workgroups' F) and lwgg as the one-pass log-sum-exp's;
    // d at the accepted point in lw, the margins of one launch in lz, f and g of a weights pass in lscal and lgpart
    DevBuf<double> lw_trial; // d of the evaluations that are not a weights pass (trial points): written, never read
    DevBuf<double> lzero;    // n_pad zeros: what the Hessian-vector product's kernels take where log-sum-exp has gbar
    // sparse logistic (qn_sparse_logistic.hip.h): A and A' in CSR (sp_nnz entries each), yw in b (m); lw, lw_trial, lzero, lgpart, lscal as the logistic's
    QnSlogCsr sl_a, sl_at;
    DevBuf<double> sl_coef, sl_t; // m each: -(yw s) of one evaluation, d o (A v) of one product -- what the column pass gathers
    // multinomial (qn_multinomial.hip.h): A rows in Q ([mrpr][mn_nfp]), the weights in b (m_pad), n = K n_features (class-major), T its padding; lse_G, lwgms,
    // lwgg ([workgroup][N_pad]), lzero, lgpart, lscal as the logistic's; P (m_pad x K) at the accepted point in mn_P, of trial evaluations in mn_P_trial
    int mn_k = 0, mn_nf = 0, mn_nfp = 0;
    QnMnlPlan mn_plan{};
    QnMnlMfmaPlan mn_mfma{};
    int mn_kernel = 1; // the stream's kernel in use: 1 mnl_onepass_kernel (vector unit), 2 mnl_mfma_kernel (qn_multinomial_set_kernel)
    DevBuf<int> mn_lab;
    DevBuf<double> mn_P, mn_P_trial;
};

static int objective_base(qn_context* ctx, size_t n, const double* b_host, qn_objective** out) {
    if (!ctx || !out || !b_host || n == 0) return fail(QN_ERROR_INPUT_PARAMS, "null argument or n == 0");
    if (n > (size_t)1 << 30) return fail(QN_ERROR_INPUT_PARAMS, "n too large");
    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    o->ctx = ctx;
    o->kind = OBJ_QUADRATIC;
    o->n = n;
    o->T = make_tile(n, ctx, 1);
    *out = o;
    QNCHK(o->Q.alloc_zero((size_t)o->T.rpr * o->T.n_pad, ctx->stream));
    QNCHK(o->b.alloc_zero(o->T.n_pad, ctx->stream));
    HIPCHK(hipMemcpyAsync(o->b, b_host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
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
        HIPCHK(hipMemcpy2D(o->Q, (size_t)o->T.n_pad * sizeof(double), q_host + r0 * n, n * sizeof(double), n * sizeof(double), nr,
                           hipMemcpyHostToDevice));
    }
    // g = Q x - b is the gradient of f only for a symmetric Q, but nothing stops a caller from passing another matrix: the row
    // kernels multiply by what was given, so the symmetric-storage evaluation is used only when Q is symmetric bit for bit
    for (size_t i = 0; i < n && o->q_symmetric; ++i)
        for (size_t j = i + 1; j < n; ++j)
            if (q_host[i * n + j] != q_host[j * n + i]) { o->q_symmetric = false; break; }
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
    hipLaunchKernelGGL(synth_fill_kernel, dim3(2048), dim3(256), 0, ctx->stream, o->Q, o->T, seed, diag, 1.0 / (double)n);
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
    o->ctx = ctx; o->kind = OBJ_LOGSUMEXP; o->n = n; o->m = m; o->mu = mu;
    o->T = make_tile(n, ctx, 1);  // column padding follows the solver's vectors
    o->TA = make_tile(m, ctx, 1); // rows of A are sharded
    const size_t np = o->T.n_pad, mp = o->TA.n_pad, mrpr = o->TA.rpr;
    hipStream_t st = ctx->stream;
    QNCHK(o->Q.alloc_zero(mrpr * np, st));
    QNCHK(o->b.alloc_zero(mp, st));
    HIPCHK(hipMemcpyAsync(o->b, c_host, m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // the zero-fill above must land before the (null-stream) 2-D upload below
    const size_t r0 = (size_t)o->TA.row_off;
    if (r0 < m) {
        const size_t nr = std::min(mrpr, m - r0);
        HIPCHK(hipMemcpy2D(o->Q, np * sizeof(double), a_host + r0 * n, n * sizeof(double), n * sizeof(double), nr, hipMemcpyHostToDevice));
    }
    o->lse_rs = (int)std::max<size_t>(1, std::min<size_t>(64, mrpr / 64));
    QNCHK(o->lz.alloc_zero((size_t)ctx->world * 2 * mrpr, st));
    QNCHK(o->lw.alloc_zero(mp, st));
    QNCHK(o->lgpart.alloc_zero((size_t)o->lse_rs * np, st));
    QNCHK(o->lgall.alloc_zero((size_t)ctx->world * np, st));
    QNCHK(o->lscal.alloc_zero(2, st));
    o->lse_two_pass = getenv("QN_LSE_TWO_PASS") && atoi(getenv("QN_LSE_TWO_PASS")) != 0;
    if (np <= 16384 && np >= 2) { // the one-pass evaluation keeps a whole row per workgroup in registers
        int kch = 1;
        while ((size_t)kch * 1024 < np) kch *= 2;
        o->lse_kch = kch;
        o->lse_G = (int)std::max<size_t>(1, std::min<size_t>(256, (mrpr + 3) / 4));
        QNCHK(o->lwgms.alloc_zero(2 * (size_t)o->lse_G, st));
        QNCHK(o->lwgg.alloc_zero((size_t)o->lse_G * np, st));
        QNCHK(o->lms.alloc_zero(2 * (size_t)ctx->world, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return QN_OK;
}

// ---- the sparse quadratic: f = 1/2 x'Qx - b'x with Q in CSR (kernels and the evaluation's launches: qn_sparse.hip.h) ----
static int spq_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, int which = 3);
// ---- the logistic objective (kernels: qn_logistic.hip.h; creation and these launches: qn_host_logistic.hip.h) ----
static int logit_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, double* d_dev, int which = 3);
static int logit_enqueue_weights(qn_objective* o, const double* x_dev);
static int logit_hess_vec_at(qn_objective* o, const double* x_host, const double* v_host, double* q_host, double* vhv);
// ---- the sparse logistic objective (kernels: qn_sparse_logistic.hip.h; creation and these launches: qn_host_sparse_logistic.hip.h) ----
static int slog_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, double* d_dev, int which = 3);
static int slog_enqueue_weights(qn_objective* o, const double* x_dev);
static int slog_hess_vec_at(qn_objective* o, const double* x_host, const double* v_host, double* q_host, double* vhv);
static uint64_t slog_eval_bytes(const qn_objective* o);
static uint64_t slog_product_bytes(const qn_objective* o);
// ---- the multinomial objective (kernel: qn_multinomial.hip.h; creation and these launches: qn_host_multinomial.hip.h) ----
struct QnVecCtl;
static int mnl_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, double* p_dev, int which = 3);
static int mnl_enqueue_weights(qn_objective* o, const double* x_dev);
static int mnl_enqueue_hess_vec(qn_objective* o, const double* v_dev, double* q_dev, const QnVecCtl* ctl, int which = 3);
static int mnl_hess_vec_at(qn_objective* o, const double* x_host, const double* v_host, double* q_host, double* vhv);

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

// lanes per row from the mean row length: the largest power of two that is at most half of it (1 .. 64).  Measured (tools/bench_sparse.py):
// the five-point Laplacian (5 per row) is fastest with 2 lanes, a random pattern of 17 per row with 16 to 32 (8 lanes: 9 % behind)
static int spq_auto_lanes(size_t n, size_t nnz) {
    const double mean = (double)nnz / (double)n;
    int L = 1;
    while (L < 64 && (double)(2 * L) <= 0.5 * mean) L *= 2;
    return L;
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
    // the device's copy: int32 whatever came in
    std::vector<int> rp(n + 1), ci(std::max<size_t>(nnz, 1), 0);
    if (index_bytes == 4) {
        memcpy(rp.data(), row_ptr_host, (n + 1) * sizeof(int));
        if (nnz) memcpy(ci.data(), col_idx_host, nnz * sizeof(int));
    } else {
        const int64_t *r8 = (const int64_t*)row_ptr_host, *c8 = (const int64_t*)col_idx_host;
        for (size_t i = 0; i <= n; ++i) rp[i] = (int)r8[i];
        for (size_t j = 0; j < nnz; ++j) ci[j] = (int)c8[j];
    }
    // symmetry, bit for bit: the transpose by a counting sort (its rows come out with increasing columns), compared with what was given
    bool symmetric = true;
    {
        std::vector<int> tp(n + 1, 0);
        for (size_t j = 0; j < nnz; ++j) tp[(size_t)ci[j] + 1]++;
        for (size_t i = 0; i < n; ++i) tp[i + 1] += tp[i];
        symmetric = memcmp(tp.data(), rp.data(), (n + 1) * sizeof(int)) == 0;
        if (symmetric && nnz) {
            std::vector<int> fill(tp.begin(), tp.end() - 1), tc(nnz);
            std::vector<double> tv(nnz);
            for (size_t i = 0; i < n; ++i)
                for (int j = rp[i]; j < rp[i + 1]; ++j) {
                    const int k = fill[(size_t)ci[j]]++;
                    tc[(size_t)k] = (int)i;
                    tv[(size_t)k] = values_host[j];
                }
            symmetric = memcmp(tc.data(), ci.data(), nnz * sizeof(int)) == 0 && memcmp(tv.data(), values_host, nnz * sizeof(double)) == 0;
        }
    }
    // the static cut: workgroup w takes the rows whose prefix weight (nonzeros + rows in front of them) falls into its G-th of the total
    const size_t total = nnz + n;
    const int G = (int)std::min<size_t>(SPQ_MAXG, std::max<size_t>(1, (total + 4095) / 4096));
    std::vector<int> cut((size_t)G + 1), longs;
    for (int w = 0; w <= G; ++w) {
        const uint64_t target = (uint64_t)total * (uint64_t)w / (uint64_t)G;
        size_t lo = 0, hi = n; // the first row i with row_ptr[i] + i >= target
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if ((uint64_t)rp[mid] + mid >= target) hi = mid; else lo = mid + 1;
        }
        cut[(size_t)w] = (int)lo;
    }
    cut[0] = 0; cut[(size_t)G] = (int)n;
    for (size_t i = 0; i < n; ++i)
        if (rp[i + 1] - rp[i] > SPQ_LONG_ROW) longs.push_back((int)i);

    HIPCHK(hipSetDevice(ctx->device));
    qn_objective* o = new qn_objective();
    *out = o;
    o->ctx = ctx; o->kind = OBJ_SPARSE_QUADRATIC; o->n = n;
    o->T = make_tile(n, ctx, 1); // (the padding of the solver's vectors)
    o->q_symmetric = symmetric;
    o->sp_nnz = nnz; o->sp_n_long = longs.size(); o->sp_G = G;
    o->sp_lanes = o->sp_lanes_auto = spq_auto_lanes(n, nnz);
    hipStream_t st = ctx->stream;
    QNCHK(o->b.alloc_zero(o->T.n_pad, st));
    QNCHK(o->sp_row_ptr.alloc(n + 1));
    QNCHK(o->sp_col.alloc(std::max<size_t>(nnz, 1)));
    QNCHK(o->sp_val.alloc_zero(std::max<size_t>(nnz, 1), st));
    QNCHK(o->sp_wg_row_start.alloc((size_t)G + 1));
    QNCHK(o->sp_long_rows.alloc(std::max<size_t>(longs.size(), 1)));
    QNCHK(o->sp_part.alloc_zero((size_t)G + longs.size(), st));
    HIPCHK(hipMemcpyAsync(o->b, b_host, n * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->sp_row_ptr, rp.data(), (n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->sp_col, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (nnz) HIPCHK(hipMemcpyAsync(o->sp_val, values_host, nnz * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->sp_wg_row_start, cut.data(), cut.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!longs.empty()) HIPCHK(hipMemcpyAsync(o->sp_long_rows, longs.data(), longs.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // (the staging vectors above go out of scope)
    return QN_OK;
}

extern "C" int qn_sparse_quadratic_set_lanes_per_row(qn_objective* o, int lanes) {
    if (!o || o->kind != OBJ_SPARSE_QUADRATIC) return fail(QN_ERROR_INPUT_PARAMS, "lanes_per_row belongs to a sparse quadratic");
    if (lanes == 0) { o->sp_lanes = o->sp_lanes_auto; return QN_OK; }
    if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1)) != 0)
        return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: lanes_per_row must be 0 (automatic), 1, 2, 4, 8, 16, 32 or 64");
    o->sp_lanes = lanes;
    return QN_OK;
}

extern "C" int qn_objective_sparse_info(qn_objective* o, size_t* nnz, int* lanes_per_row, size_t* n_long_rows, int* symmetric) {
    if (o && o->kind == OBJ_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "a logistic objective is not a sparse quadratic (its A is dense)");
    if (o && o->kind == OBJ_SPARSE_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "a sparse logistic objective is not a sparse quadratic: qn_sparse_logistic_info describes it");
    if (o && o->kind == OBJ_MULTINOMIAL) return fail(QN_ERROR_INPUT_PARAMS, "a multinomial objective is not a sparse quadratic (its A is dense)");
    if (!o || o->kind != OBJ_SPARSE_QUADRATIC) return fail(QN_ERROR_INPUT_PARAMS, "not a sparse quadratic");
    if (nnz) *nnz = o->sp_nnz;
    if (lanes_per_row) *lanes_per_row = o->sp_lanes;
    if (n_long_rows) *n_long_rows = o->sp_n_long;
    if (symmetric) *symmetric = o->q_symmetric ? 1 : 0;
    return QN_OK;
}

template <int R>
static void launch_hpass(hipStream_t st, const QnHPassArgs& a);

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

// the first launches of the two-pass evaluation at x_dev: z = A_rows x, the softmax weights NORMALISED into `lw` (zero past row m), this rank's
// column sums A'w into its block of `lgall`, f's terms into `lscal` -- what lse_finish_kernel needs, and what the Hessian needs (p and gbar)
static int lse_enqueue_weights(qn_objective* o, const double* x_dev, QnLseArgs& a) {
    qn_context* c = o->ctx;
    hipStream_t st = c->stream;
    // pass 1: z = A_rows x (the H-pass kernel in plain mat-vec mode)
    QnHPassArgs h{};
    h.H = o->Q; h.T = o->TA; h.T.n_pad = o->T.n_pad; h.T.n = (int)o->n; h.T.cs = 1;
    h.T.rpr = o->TA.rpr; h.T.row_off = 0; // row guards are not needed for a read-only pass
    h.hp = o->lz; h.expect_phase = -1; h.force_nrhs = 1; h.force_pending = 0; h.r0 = x_dev; h.r1 = x_dev;
    h.sp = x_dev; h.up = x_dev;
    launch_hpass<8>(st, h);
    HIPCHK(hipGetLastError());
    c->n_xchg_vector++;
    QNCHK(exchange(c, o->lz, 2 * (size_t)o->TA.rpr));
    a = QnLseArgs{};
    a.A = o->Q; a.c = o->b; a.z = o->lz; a.w = o->lw; a.gpart = o->lgpart; a.gall = o->lgall; a.x = x_dev;
    a.scal = o->lscal; a.mu = o->mu;
    a.m = (int)o->m; a.m_pad = o->TA.n_pad; a.mrpr = o->TA.rpr; a.n = (int)o->n; a.n_pad = o->T.n_pad;
    a.world = c->world; a.rank = c->rank; a.rs = o->lse_rs;
    hipLaunchKernelGGL(lse_softmax_kernel, dim3(1), dim3(1024), 0, st, a);
    // pass 2: column sums A'w over this rank's rows
    hipLaunchKernelGGL(lse_colsum_kernel, dim3((a.n_pad + QN_CHUNK - 1) / QN_CHUNK, a.rs), dim3(QN_TPB), 0, st, a);
    hipLaunchKernelGGL(lse_reduce_splits_kernel, dim3(std::min(1024, (a.n_pad + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

static int lse_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev) {
    qn_context* c = o->ctx;
    hipStream_t st = c->stream;
    if (o->lse_kch && !o->lse_two_pass) { // one pass over A (qn_kernels.hip.h): 8 m n / P bytes per evaluation instead of 16 m n / P
        QnLseArgs a{};
        a.A = o->Q; a.c = o->b; a.gall = o->lgall; a.x = x_dev; a.f_out = f_dev; a.g_out = g_dev; a.mu = o->mu;
        a.m = (int)o->m; a.m_pad = o->TA.n_pad; a.mrpr = o->TA.rpr; a.n = (int)o->n; a.n_pad = o->T.n_pad;
        a.world = c->world; a.rank = c->rank; a.rs = 1;
        int lst;
        switch (o->lse_kch) {
        case 1: lst = lse_launch_onepass<1>(st, o->lse_G, a, o->lwgms, o->lwgg); break;
        case 2: lst = lse_launch_onepass<2>(st, o->lse_G, a, o->lwgms, o->lwgg); break;
        case 4: lst = lse_launch_onepass<4>(st, o->lse_G, a, o->lwgms, o->lwgg); break;
        case 8: lst = lse_launch_onepass<8>(st, o->lse_G, a, o->lwgms, o->lwgg); break;
        default: lst = lse_launch_onepass<16>(st, o->lse_G, a, o->lwgms, o->lwgg); break;
        }
        if (lst < 0) { o->lse_two_pass = 1; return lse_enqueue_eval(o, x_dev, f_dev, g_dev); }
        hipLaunchKernelGGL(lse_combine_kernel, dim3((a.n_pad + 63) / 64), dim3(256), 0, st, a, o->lse_G, o->lwgms, o->lwgg, o->lms);
        HIPCHK(hipGetLastError());
        const XchgItem items[2] = {{o->lgall, (size_t)a.n_pad}, {o->lms, 2}};
        c->n_xchg_vector++;
        QNCHK(exchange_group(c, items, 2));
        hipLaunchKernelGGL(lse_finish1_kernel, dim3(std::min(1024, (a.n_pad + 255) / 256)), dim3(256), 0, st, a, o->lms);
        HIPCHK(hipGetLastError());
        return QN_OK;
    }
    QnLseArgs a{};
    QNCHK(lse_enqueue_weights(o, x_dev, a));
    a.f_out = f_dev; a.g_out = g_dev;
    c->n_xchg_vector++;
    QNCHK(exchange(c, o->lgall, (size_t)a.n_pad));
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
    QNCHK(lse_enqueue_weights(o, x_dev, a)); // p -> lw, gbar -> lgall (rank 0's block is the whole sum on one rank)
    return lse_hess_launch(o->ctx->stream, o->Q, o->lw, o->lgall, o->mu, (int)o->m, o->T.n_pad, h_dev, ld);
}

extern "C" void qn_objective_destroy(qn_objective* o) {
    if (!o) return;
    (void)hipSetDevice(o->ctx->device);
    delete o;
}

extern "C" int qn_objective_get_rows(qn_objective* o, size_t row0, size_t nrows, double* out_host) {
    if (o->kind == OBJ_SPARSE_QUADRATIC) return fail(QN_ERROR_INPUT_PARAMS, "a sparse quadratic has no dense rows / Hessian");
    if (o->kind == OBJ_SPARSE_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "a sparse logistic objective has no dense rows / Hessian");
    if (o->kind == OBJ_MULTINOMIAL) return fail(QN_ERROR_INPUT_PARAMS, "get_rows is not built for a multinomial objective (its n is K n_features, not the width of A)");
    if (o->kind != OBJ_QUADRATIC && o->kind != OBJ_LOGSUMEXP && o->kind != OBJ_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "unsupported objective");
    const bool lse = o->kind == OBJ_LOGSUMEXP || o->kind == OBJ_LOGISTIC; // (rows of the dense A)
    const size_t lo = lse ? (size_t)o->TA.row_off : (size_t)o->T.row_off;
    const size_t hi = lse ? std::min(o->m, lo + (size_t)o->TA.rpr) : std::min(o->n, lo + (size_t)o->T.rpr);
    if (row0 < lo || row0 + nrows > hi) return fail(QN_ERROR_INPUT_PARAMS, "rows outside this rank's shard");
    HIPCHK(hipSetDevice(o->ctx->device));
    HIPCHK(hipMemcpy2D(out_host, o->n * sizeof(double), o->Q + (row0 - lo) * (size_t)o->T.n_pad, (size_t)o->T.n_pad * sizeof(double),
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

extern "C" int qn_objective_eval(qn_objective* o, const double* x_host, double* f, double* g_host) {
    qn_context* c = o->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t np = o->T.n_pad;
    if (o->kind == OBJ_LOGSUMEXP) {
        QNCHK(o->ex.ensure(2 * np, c->stream));
        QNCHK(o->eg.ensure(np, c->stream));
        QNCHK(o->ef.ensure(2, c->stream));
        HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        QNCHK(lse_enqueue_eval(o, o->ex, o->ef, o->eg));
        HIPCHK(hipMemcpyAsync(f, o->ef, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(g_host, o->eg, o->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return QN_OK;
    }
    if (o->kind == OBJ_SPARSE_QUADRATIC || o->kind == OBJ_LOGISTIC || o->kind == OBJ_SPARSE_LOGISTIC || o->kind == OBJ_MULTINOMIAL) {
        QNCHK(o->ex.ensure(2 * np, c->stream));
        QNCHK(o->eg.ensure(np, c->stream));
        QNCHK(o->ef.ensure(2, c->stream));
        HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (o->kind == OBJ_LOGISTIC) QNCHK(logit_enqueue_eval(o, o->ex, o->ef, o->eg, o->lw_trial)); // (lw keeps the last weights pass's d)
        else if (o->kind == OBJ_SPARSE_LOGISTIC) QNCHK(slog_enqueue_eval(o, o->ex, o->ef, o->eg, o->lw_trial));
        else if (o->kind == OBJ_MULTINOMIAL) QNCHK(mnl_enqueue_eval(o, o->ex, o->ef, o->eg, o->mn_P_trial)); // (mn_P keeps the last weights pass's P)
        else QNCHK(spq_enqueue_eval(o, o->ex, o->ef, o->eg));
        HIPCHK(hipMemcpyAsync(f, o->ef, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(g_host, o->eg, o->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return QN_OK;
    }
    if (o->kind != OBJ_QUADRATIC) return fail(QN_ERROR_INPUT_PARAMS, "unsupported objective");
    QNCHK(o->ex.ensure(2 * np, c->stream)); // x and xt
    QNCHK(o->eq.ensure(np, c->stream));
    QNCHK(o->eg.ensure(np, c->stream));
    QNCHK(o->ef.ensure(2, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QnQuadArgs a{};
    a.Q = o->Q; a.T = o->T; a.x = o->ex; a.d = o->ex; a.xt = o->ex + np;
    a.out = o->eq + (size_t)c->rank * o->T.rpr;
    a.ctl = nullptr; a.expect_phase = -1; a.force_kind = QN_REQ_X; a.force_t = 0.0;
    QNCHK(launch_quad_R(8, c->stream, a));
    QNCHK(exchange(c, o->eq, (size_t)o->T.rpr));
    QnVecs V{};
    V.q = o->eq; V.xt = o->ex + np; V.b = o->b; V.n = (int)o->n; V.n_pad = (int)np; V.rpr = o->T.rpr; V.world = c->world; V.qcs = 1; V.hcs = 1;
    hipLaunchKernelGGL(quad_finish_kernel, dim3(1), dim3(QN_CTL_TPB), 0, c->stream, V, o->ef, o->eg);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(f, o->ef, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(g_host, o->eg, o->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return QN_OK;
}

extern "C" int qn_objective_hessian(qn_objective* o, const double* x_host, double* h_colmajor_host) {
    if (!o || !x_host) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (o->kind == OBJ_SPARSE_QUADRATIC) return fail(QN_ERROR_INPUT_PARAMS, "a sparse quadratic has no dense rows / Hessian");
    if (o->kind == OBJ_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "the dense Hessian of a logistic objective is not built: hess_vec_at gives H(x) v in one stream of A");
    if (o->kind == OBJ_SPARSE_LOGISTIC) return fail(QN_ERROR_INPUT_PARAMS, "a sparse logistic objective has no dense rows / Hessian: hess_vec_at gives H(x) v");
    if (o->kind == OBJ_MULTINOMIAL) return fail(QN_ERROR_INPUT_PARAMS, "the dense Hessian of a multinomial objective is not built: hess_vec_at gives H(x) v in one stream of A");
    qn_context* c = o->ctx;
    if (c->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "qn_objective_hessian is single-GPU");
    HIPCHK(hipSetDevice(c->device));
    const size_t n = o->n, np = o->T.n_pad;
    if (o->kind == OBJ_QUADRATIC) { // Q itself, whatever x is
        if (!h_colmajor_host) return QN_OK;
        std::vector<double> rows(n * n);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy2D(rows.data(), n * sizeof(double), o->Q, np * sizeof(double), n * sizeof(double), n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < n; ++j) h_colmajor_host[i + j * n] = rows[i * n + j];
        return QN_OK;
    }
    if (o->kind != OBJ_LOGSUMEXP) return fail(QN_ERROR_INPUT_PARAMS, "unsupported objective");
    QNCHK(o->ex.ensure(2 * np, c->stream));
    QNCHK(o->eh.ensure(np * np));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(lse_enqueue_hessian(o, o->ex, o->eh, np));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!h_colmajor_host) return QN_OK; // (the launches alone: what tools/bench_lse_hessian.py times)
    // H == H' bit for bit: its rows are its columns
    HIPCHK(hipMemcpy2D(h_colmajor_host, n * sizeof(double), o->eh, np * sizeof(double), n * sizeof(double), n, hipMemcpyDeviceToHost));
    return QN_OK;
}
