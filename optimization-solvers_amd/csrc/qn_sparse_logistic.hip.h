// qn_sparse_logistic.hip.h -- the sparse logistic-regression objective (OBJ_SPARSE_LOGISTIC) on a CSR A (m x n, one rank, no limit on n_pad):
//
//     f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2,      g = -A'(y o w o s) + mu x,      H(x) v = A'(d o (A v)) + mu v
//
// The device holds TWO CSR copies, A and A' (int32 offsets, int32 columns, f64 values: 24 bytes per nonzero): the transpose product walks the rows
// of A' with the kernel that walks the rows of A, so no float atomic is needed and every sum has one fixed order.  Each copy has its own static
// cut, its own list of long rows and its own lanes per row (SparseQuadratic's rules, qn_csr_host.h).  A dense column of A -- an intercept column
// of ones -- is a long row of A' and gets a whole workgroup.
//
//   slog_rows_kernel<L, PRODUCT>   spq_eval_kernel's geometry (qn_sparse.hip.h) over the rows of A: L consecutive lanes own a row, lane l adds the
//                                  products of entries l, l + L, ... in that order, the xor tree L/2 .. 1; a workgroup walks its range of the cut
//                                  256 / L rows per trip; a row of more than SPQ_LONG_ROW entries is summed by workgroup G + k of the same launch
//                                  (thread t: entries t, t + 256, ...; then the block sum).  With u_i = a_i . x, lane 0 of the row:
//                                    evaluation  z = sign(yw) u; t = |z|; e = exp(-t); q = 1 + e; s = (z >= 0 ? e : 1) / q; coef = -(yw s);
//                                                d = |yw| ((e / q) / q); l = |yw| (max(-z, 0) + log1p(e)); yw = 0: coef = d = l = 0 by selects
//                                                (logit_onepass_kernel's formulas and order); coef_i and d_i are stored, l_i is added to the
//                                                lane's sum (plain adds, the rows of the lane in index order), and the workgroup leaves ONE
//                                                share of sum l_i (block sum)
//                                    product     t_i = d_i u_i (one rounding) with u_i = a_i . v and the stored d; no transcendental function
//   slog_cols_kernel<L, PRODUCT>   the same geometry over the rows of A' (the columns of A), gathering the m-vector the row pass stored:
//                                    evaluation  g_j = (sum_i a_ij coef_i) + mu x_j  and the workgroup's share of sum x_j^2
//                                    product     q_j = (sum_i a_ij t_i) + mu v_j     and the workgroup's share of sum v_j q_j
//                                  (mu x_j rounds on its own; x_j^2 and v_j q_j round before they are added).  Entries n .. n_pad are never written.
//   slog_finish_kernel             (1 workgroup) spq_finish_kernel's strided order: thread j adds shares j, j + 256, ..., then the block sum.
//                                    evaluation  f = sum(loss shares) + 0.5 mu sum(xx shares)
//                                    product     the shares of v'Hv folded into ONE value: tn_step_kernel adds at most 256 shares, a column cut
//                                                has up to SPQ_MAXG + n_long, so NewtonCG reads this value with kcount = 1
//
// No atomics, no workgroup waits for another, every order is fixed by (pattern, L): the same bits from run to run and from object to object.
// Products and sums round separately (-ffp-contract=off).  Product launches take `ctl`: non-null, they return at once unless QN_NEWTON_CG's inner
// loop is running (lse_hv_onepass_kernel's predicate); null, they always run.
//
// ADDRESSING: 32-bit element indices (nnz <= 2^31 - 1, m, n <= 2^30, checked at creation).  Nothing is read past row_ptr[rows]; columns were
// checked against the other dimension on the host, and the transpose's columns are row numbers of A by construction.  A wave's loads of values
// and columns are contiguous; the gathers of x / coef / t bound the kernels (they rely on L2 and the Infinity Cache, as spq_eval_kernel's do).
#pragma once

struct QnSlogArgs {
    const int* row_ptr;      // rows + 1 of the copy this launch walks
    const int* col;          // nnz
    const double* val;       // nnz
    const int* wg_row_start; // G + 1
    const int* long_rows;    // n_long
    const double* src;       // the gathered vector: x or v (row pass), coef or t (column pass)
    const double* yw;        // row pass, evaluation: y o w (m)
    const double* d_in;      // row pass, product: d at the weights' point (m)
    const double* xv;        // column pass: x (evaluation) or v (product), n entries read
    double* out;             // row pass: coef (evaluation) or t (product), m; column pass: g or q, n entries written
    double* d_out;           // row pass, evaluation: d (m)
    double* part;            // G + n_long shares (row pass evaluation: loss; column pass: x.x or v.q)
    double mu;
    int G, n_long;
};

__device__ __forceinline__ bool slog_skip(const QnVecCtl* ctl) {
    return ctl && (ctl->phase != QN_VP_NSOLVE || ctl->method != QN_NEWTON_CG || ctl->tn_state != QN_TN_RUNNING);
}

__device__ __forceinline__ double slog_product(const QnSlogArgs& a, int j) { return a.val[j] * a.src[a.col[j]]; }

// what lane 0 of row i does with u = a_i . src; returns the row's term of the workgroup's share
template <bool PRODUCT>
__device__ __forceinline__ double slog_row_end(const QnSlogArgs& a, int i, double u) {
    if (PRODUCT) {
        a.out[i] = a.d_in[i] * u;
        return 0.0;
    }
    const double ywr = a.yw[i];
    const double z = ywr < 0.0 ? -u : u;
    const double t = fabs(z);
    const double e = exp(-t);
    const double q = 1.0 + e;
    const double s = (z >= 0.0 ? e : 1.0) / q;
    const double ys = ywr * s;
    const double aw = fabs(ywr);
    const double dr = aw * ((e / q) / q);
    const double lr = aw * (fmax(-z, 0.0) + log1p(e));
    const bool live = ywr != 0.0; // (selects, not branches: a masked row adds nothing even where its u overflowed from finite entries)
    a.out[i] = live ? -ys : 0.0;
    a.d_out[i] = live ? dr : 0.0;
    return live ? lr : 0.0;
}

template <bool PRODUCT>
__device__ __forceinline__ double slog_col_end(const QnSlogArgs& a, int j, double acc) {
    const double xj = a.xv[j];
    const double mx = a.mu * xj;
    const double gj = acc + mx;
    a.out[j] = gj;
    return PRODUCT ? xj * gj : xj * xj;
}

template <int L, bool PRODUCT, bool COLS>
__device__ __forceinline__ void slog_pass(const QnSlogArgs& a, double* lds) {
    double fs[1] = {0.0};
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.G) { // one long row, the whole workgroup
        const int i = a.long_rows[blockIdx.x - a.G];
        const int j1 = a.row_ptr[i + 1];
        double acc[1] = {0.0};
        for (int j = a.row_ptr[i] + tid; j < j1; j += SPQ_TPB) acc[0] = acc[0] + slog_product(a, j);
        ctl_block_sum<1>(acc, lds);
        if (tid == 0) {
            const double term = COLS ? slog_col_end<PRODUCT>(a, i, acc[0]) : slog_row_end<PRODUCT>(a, i, acc[0]);
            if (COLS || !PRODUCT) a.part[blockIdx.x] = term;
        }
        return;
    }
    constexpr int RPT = SPQ_TPB / L; // rows per trip
    const int r0 = a.wg_row_start[blockIdx.x], r1 = a.wg_row_start[blockIdx.x + 1];
    const int sub = tid / L, l = tid % L;
    for (int base = r0; base < r1; base += RPT) {
        const int i = base + sub;
        int j0 = 0, j1 = 0;
        if (i < r1) { j0 = a.row_ptr[i]; j1 = a.row_ptr[i + 1]; }
        const bool regular = j1 - j0 <= SPQ_LONG_ROW; // (a long row: nothing here, its own workgroup stores its results and its share)
        double acc = 0.0;
        if (regular)
            for (int j = j0 + l; j < j1; j += L) acc = acc + slog_product(a, j);
#pragma unroll
        for (int off = L / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        if (l == 0 && i < r1 && regular) {
            const double term = COLS ? slog_col_end<PRODUCT>(a, i, acc) : slog_row_end<PRODUCT>(a, i, acc);
            fs[0] = fs[0] + term;
        }
    }
    if (COLS || !PRODUCT) { // (the row pass of a product leaves no share)
        ctl_block_sum<1>(fs, lds);
        if (tid == 0) a.part[blockIdx.x] = fs[0];
    }
}

template <int L, bool PRODUCT>
__global__ __launch_bounds__(SPQ_TPB) void slog_rows_kernel(const QnSlogArgs a, const QnVecCtl* ctl) {
    __shared__ double lds[16];
    if (PRODUCT && slog_skip(ctl)) return;
    slog_pass<L, PRODUCT, false>(a, lds);
}

template <int L, bool PRODUCT>
__global__ __launch_bounds__(SPQ_TPB) void slog_cols_kernel(const QnSlogArgs a, const QnVecCtl* ctl) {
    __shared__ double lds[16];
    if (PRODUCT && slog_skip(ctl)) return;
    slog_pass<L, PRODUCT, true>(a, lds);
}

// product == 0: *out = sum(lpart[0 .. lcount)) + 0.5 mu sum(xpart[0 .. xcount));  product != 0: *out = sum(xpart[0 .. xcount)), predicated on ctl
__global__ __launch_bounds__(SPQ_TPB) void slog_finish_kernel(const double* lpart, int lcount, const double* xpart, int xcount, double mu, double* out,
                                                              const QnVecCtl* ctl, int product) {
    __shared__ double lds[32];
    if (product && slog_skip(ctl)) return;
    double v[2] = {0.0, 0.0};
    if (!product)
        for (int b = threadIdx.x; b < lcount; b += SPQ_TPB) v[0] = v[0] + lpart[b];
    for (int b = threadIdx.x; b < xcount; b += SPQ_TPB) v[1] = v[1] + xpart[b];
    ctl_block_sum<2>(v, lds);
    if (threadIdx.x == 0) *out = product ? v[1] : v[0] + 0.5 * mu * v[1];
}

template <int L, bool PRODUCT, bool COLS>
static void slog_launch_L(hipStream_t st, const QnSlogArgs& a, const QnVecCtl* ctl) {
    if (COLS) hipLaunchKernelGGL((slog_cols_kernel<L, PRODUCT>), dim3(a.G + a.n_long), dim3(SPQ_TPB), 0, st, a, ctl);
    else hipLaunchKernelGGL((slog_rows_kernel<L, PRODUCT>), dim3(a.G + a.n_long), dim3(SPQ_TPB), 0, st, a, ctl);
}

template <bool PRODUCT, bool COLS>
static int slog_launch(hipStream_t st, const QnSlogArgs& a, int lanes, const QnVecCtl* ctl) {
    switch (lanes) {
    case 1: slog_launch_L<1, PRODUCT, COLS>(st, a, ctl); break;
    case 2: slog_launch_L<2, PRODUCT, COLS>(st, a, ctl); break;
    case 4: slog_launch_L<4, PRODUCT, COLS>(st, a, ctl); break;
    case 8: slog_launch_L<8, PRODUCT, COLS>(st, a, ctl); break;
    case 16: slog_launch_L<16, PRODUCT, COLS>(st, a, ctl); break;
    case 32: slog_launch_L<32, PRODUCT, COLS>(st, a, ctl); break;
    case 64: slog_launch_L<64, PRODUCT, COLS>(st, a, ctl); break;
    default: return fail(QN_ERROR_INPUT_PARAMS, "sparse logistic: lanes must be 1, 2, 4, 8, 16, 32 or 64");
    }
    return QN_OK;
}

// ---- the diagonal of the Hessian: M_j = sum_{i in column j} d_i a_ij^2 + mu over A' (what NewtonCG's Jacobi preconditioner divides by) ----
//   slog_diag_kernel<L>   slog_cols_kernel's sibling: the same geometry over the rows of A' (the static cut, L lanes per row, the xor tree L/2 .. 1,
//                         a long row summed by workgroup G + k, thread t: entries t, t + 256, ...; then the block sum).  THE ROUNDING ORDER, per
//                         entry: s = val val (rounded), then s d[col] (rounded), added in the pass's order (plain adds).  M_j = acc + mu; where
//                         `minv` is not NULL the same launch writes 1 / M_j by IEEE division when M_j > 0 and finite, else 1 (hd_minv).  An empty
//                         column gives M_j = mu.  No shares, no finish launch, unpredicated; entries n .. n_pad are never written.
struct QnSlogDiagArgs {
    const int* row_ptr;      // n + 1: the rows of A'
    const int* col;          // nnz: row numbers of A
    const double* val;       // nnz
    const int* wg_row_start; // G + 1
    const int* long_rows;    // n_long
    const double* d;         // the weights of the last pass (m)
    double* m_out;           // n entries written
    double* minv_out;        // n entries written, or NULL
    double mu;
    int G, n_long;
};

__device__ __forceinline__ double slog_diag_product(const QnSlogDiagArgs& a, int j) {
    const double v = a.val[j];
    const double s = v * v;
    return s * a.d[a.col[j]];
}

__device__ __forceinline__ void slog_diag_end(const QnSlogDiagArgs& a, int j, double acc) {
    const double mj = acc + a.mu;
    a.m_out[j] = mj;
    if (a.minv_out) a.minv_out[j] = hd_minv(mj);
}

template <int L>
__global__ __launch_bounds__(SPQ_TPB) void slog_diag_kernel(const QnSlogDiagArgs a) {
    __shared__ double lds[16];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.G) { // one long row of A' (a dense column of A), the whole workgroup
        const int i = a.long_rows[blockIdx.x - a.G];
        const int j1 = a.row_ptr[i + 1];
        double acc[1] = {0.0};
        for (int j = a.row_ptr[i] + tid; j < j1; j += SPQ_TPB) acc[0] = acc[0] + slog_diag_product(a, j);
        ctl_block_sum<1>(acc, lds);
        if (tid == 0) slog_diag_end(a, i, acc[0]);
        return;
    }
    constexpr int RPT = SPQ_TPB / L; // rows per trip
    const int r0 = a.wg_row_start[blockIdx.x], r1 = a.wg_row_start[blockIdx.x + 1];
    const int sub = tid / L, l = tid % L;
    for (int base = r0; base < r1; base += RPT) {
        const int i = base + sub;
        int j0 = 0, j1 = 0;
        if (i < r1) { j0 = a.row_ptr[i]; j1 = a.row_ptr[i + 1]; }
        const bool regular = j1 - j0 <= SPQ_LONG_ROW; // (a long row: nothing here, its own workgroup stores its entry)
        double acc = 0.0;
        if (regular)
            for (int j = j0 + l; j < j1; j += L) acc = acc + slog_diag_product(a, j);
#pragma unroll
        for (int off = L / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        if (l == 0 && i < r1 && regular) slog_diag_end(a, i, acc);
    }
}

static int slog_diag_launch(hipStream_t st, const QnSlogDiagArgs& a, int lanes) {
    const dim3 grid(a.G + a.n_long), tpb(SPQ_TPB);
    switch (lanes) {
    case 1: hipLaunchKernelGGL(slog_diag_kernel<1>, grid, tpb, 0, st, a); break;
    case 2: hipLaunchKernelGGL(slog_diag_kernel<2>, grid, tpb, 0, st, a); break;
    case 4: hipLaunchKernelGGL(slog_diag_kernel<4>, grid, tpb, 0, st, a); break;
    case 8: hipLaunchKernelGGL(slog_diag_kernel<8>, grid, tpb, 0, st, a); break;
    case 16: hipLaunchKernelGGL(slog_diag_kernel<16>, grid, tpb, 0, st, a); break;
    case 32: hipLaunchKernelGGL(slog_diag_kernel<32>, grid, tpb, 0, st, a); break;
    case 64: hipLaunchKernelGGL(slog_diag_kernel<64>, grid, tpb, 0, st, a); break;
    default: return fail(QN_ERROR_INPUT_PARAMS, "sparse logistic: lanes must be 1, 2, 4, 8, 16, 32 or 64");
    }
    return QN_OK;
}
