// qn_sparse.hip.h -- the sparse quadratic objective (OBJ_SPARSE_QUADRATIC): f = 1/2 x'Qx - b'x, g = Qx - b with Q in CSR on the device, int32 row
// offsets, int32 columns and f64 values (12 bytes per nonzero).  One evaluation is two launches:
//
//   spq_eval_kernel<L>      q_i = sum_j Q_ij x_j for every row, g_i = q_i - b_i, and the workgroup's share of f = sum_i x_i (1/2 q_i - b_i)
//   spq_finish_kernel       (1 workgroup) the shares added in index order into *f
//
// ROWS TO LANES (CSR-vector).  L = lanes_per_row in {1 .. 64} consecutive lanes own one row: lane l of the group adds the products of the row's
// entries l, l + L, l + 2 L, ... in that order, and the L sums are folded by the xor tree L/2, L/4, ... 1 -- every lane of the group ends with
// the row's sum, lane 0 stores g_i.  A workgroup of 256 threads holds 256 / L rows at a time and walks its static range of rows
// [wg_row_start[b], wg_row_start[b + 1]) -- cut on the host so that every workgroup gets about the same number of nonzeros + rows -- 256 / L rows
// per trip.  Consecutive groups read consecutive rows, so a wave's loads of values and columns fall on one contiguous piece of the arrays.
//
// LONG ROWS.  A row of more than SPQ_LONG_ROW entries is skipped by the regular workgroups and summed by a whole workgroup of its own, in the
// SAME launch: workgroup G + k takes long_rows[k]; thread t adds entries t, t + 256, ...; then the block sum of qn_kernels.hip.h (wave xor tree,
// waves in index order).  The dense row of an arrow matrix does not serialise on L lanes.
//
// REDUCTIONS are fixed: the order in which a row's products are added is a function of the row's length class (regular / long) and L alone;
// f's shares are one per workgroup (regular ones first, then the long rows'), added by spq_finish_kernel as qn_vec.hip.h adds its partials:
// thread j takes b = j, j + 256, ..., then the block sum.  No floating-point atomic, no workgroup waits for another: the same bits from run
// to run and from object to object.  Products and sums round separately (the project's -ffp-contract=off).
//
// ADDRESSING: plain 32-bit element indices (nnz <= 2^31 - 1, n <= 2^30, checked at creation) into 64-bit base pointers.  Nothing is read past
// row_ptr[n]; columns were checked against [0, n) on the host.  Entries n .. n_pad of g are not written (they stay zero, as x's are).
// Values and columns are read with plain loads: non-temporal loads of the 12 nnz bytes that are read once were measured and lost.
#pragma once

#define SPQ_TPB 256 // (SPQ_MAXG, SPQ_LONG_ROW: qn_host_objective.hip.h, where the rows are cut)

struct QnSpqArgs {
    const int* row_ptr;      // n + 1
    const int* col;          // nnz
    const double* val;       // nnz
    const double* b;         // n_pad
    const int* wg_row_start; // G + 1
    const int* long_rows;    // n_long
    const double* x;
    double* g;
    double* part; // G + n_long
    int n, G, n_long;
};

__device__ __forceinline__ double spq_product(const QnSpqArgs& a, int j) { return a.val[j] * a.x[a.col[j]]; }

template <int L>
__global__ __launch_bounds__(SPQ_TPB) void spq_eval_kernel(const QnSpqArgs a) {
    __shared__ double lds[16];
    double fs[1] = {0.0};
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.G) { // one long row, the whole workgroup
        const int i = a.long_rows[blockIdx.x - a.G];
        const int j1 = a.row_ptr[i + 1];
        double acc[1] = {0.0};
        for (int j = a.row_ptr[i] + tid; j < j1; j += SPQ_TPB) acc[0] = acc[0] + spq_product(a, j);
        ctl_block_sum<1>(acc, lds);
        if (tid == 0) {
            const double bi = a.b[i];
            a.g[i] = acc[0] - bi;
            a.part[blockIdx.x] = a.x[i] * (0.5 * acc[0] - bi);
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
        const bool regular = j1 - j0 <= SPQ_LONG_ROW; // (a long row: nothing here, its own workgroup writes g_i and its share)
        double acc = 0.0;
        if (regular)
            for (int j = j0 + l; j < j1; j += L) acc = acc + spq_product(a, j);
#pragma unroll
        for (int off = L / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        if (l == 0 && i < r1 && regular) {
            const double bi = a.b[i];
            a.g[i] = acc - bi;
            fs[0] = fs[0] + a.x[i] * (0.5 * acc - bi);
        }
    }
    ctl_block_sum<1>(fs, lds);
    if (tid == 0) a.part[blockIdx.x] = fs[0];
}

__global__ __launch_bounds__(SPQ_TPB) void spq_finish_kernel(const double* part, int count, double* f_out) {
    __shared__ double lds[16];
    double v[1] = {0.0};
    for (int b = threadIdx.x; b < count; b += SPQ_TPB) v[0] = v[0] + part[b];
    ctl_block_sum<1>(v, lds);
    if (threadIdx.x == 0) *f_out = v[0];
}

template <int L>
static void spq_launch_L(hipStream_t st, const QnSpqArgs& a) {
    hipLaunchKernelGGL(spq_eval_kernel<L>, dim3(a.G + a.n_long), dim3(SPQ_TPB), 0, st, a);
}

// the launches of one evaluation on `st`: g and the shares (which & 1), then *f_dev (which & 2)
static int spq_launch(hipStream_t st, const QnSpqArgs& a, int lanes, double* f_dev, int which) {
    if (which & 1) {
        switch (lanes) {
        case 1: spq_launch_L<1>(st, a); break;
        case 2: spq_launch_L<2>(st, a); break;
        case 4: spq_launch_L<4>(st, a); break;
        case 8: spq_launch_L<8>(st, a); break;
        case 16: spq_launch_L<16>(st, a); break;
        case 32: spq_launch_L<32>(st, a); break;
        case 64: spq_launch_L<64>(st, a); break;
        default: return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: lanes_per_row must be 1, 2, 4, 8, 16, 32 or 64");
        }
    }
    if (which & 2) hipLaunchKernelGGL(spq_finish_kernel, dim3(1), dim3(SPQ_TPB), 0, st, a.part, a.G + a.n_long, f_dev);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// enqueue one evaluation of a sparse quadratic at x_dev: f -> f_dev, g -> g_dev[0 .. n).  `which`: 1 = the evaluation launch alone, 2 = the finish
// alone (the vector pump times the two apart in profiling mode: t_eval_ms is spq_eval_kernel alone, what tools/bench_sparse.py reports), 3 = both
static int spq_enqueue_eval(qn_objective* o, const double* x_dev, double* f_dev, double* g_dev, int which, const QnObjWork*) {
    QnSpqArgs a{};
    a.row_ptr = o->sp.row_ptr; a.col = o->sp.col; a.val = o->sp.val; a.b = o->sp.b; a.wg_row_start = o->sp.wg_row_start; a.long_rows = o->sp.long_rows;
    a.x = x_dev; a.g = g_dev; a.part = o->sp.part;
    a.n = (int)o->n; a.G = o->sp.G; a.n_long = (int)o->sp.n_long;
    return spq_launch(o->ctx->stream, a, o->sp.lanes, f_dev, which);
}

// ---- the curvature pass: q = Q d and the shares of c = d'Qd (qn_objective_hess_vec; QN_LS_EXACT_QUADRATIC's search, qn_vec_exact.hip.h) ----
// spq_eval_kernel's sibling with the same structure -- L lanes to a row, the same static cut, whole workgroups for the long rows behind the regular
// ones in the same launch, the same order of additions inside a row -- and so the same bits for q_i as an evaluation at d with b = 0 gives g_i.
// It reads d (in QnSpqArgs.x) where the evaluation reads x and reads no b; lane 0 stores q_i (in QnSpqArgs.g) and adds d_i * q_i, two roundings,
// to the workgroup's share; spq_finish_kernel adds the shares in index order.  Bytes: 12 nnz + 4 (n + 1) + 16 n, 8 n fewer than an evaluation.
// The evaluation kernel above is not touched: it keeps its code and its operation order.  `ctl` != NULL (the search): predicated on phase
// QN_VP_EXACT, like every launch of the vector machine; NULL (qn_objective_hess_vec): unconditional.
template <int L>
__global__ __launch_bounds__(SPQ_TPB) void spq_curv_kernel(const QnSpqArgs a, const QnVecCtl* ctl) {
    __shared__ double lds[16];
    if (ctl && ctl->phase != QN_VP_EXACT) return;
    double cs[1] = {0.0};
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.G) { // one long row, the whole workgroup
        const int i = a.long_rows[blockIdx.x - a.G];
        const int j1 = a.row_ptr[i + 1];
        double acc[1] = {0.0};
        for (int j = a.row_ptr[i] + tid; j < j1; j += SPQ_TPB) acc[0] = acc[0] + spq_product(a, j);
        ctl_block_sum<1>(acc, lds);
        if (tid == 0) {
            a.g[i] = acc[0];
            a.part[blockIdx.x] = a.x[i] * acc[0];
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
        const bool regular = j1 - j0 <= SPQ_LONG_ROW;
        double acc = 0.0;
        if (regular)
            for (int j = j0 + l; j < j1; j += L) acc = acc + spq_product(a, j);
#pragma unroll
        for (int off = L / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        if (l == 0 && i < r1 && regular) {
            a.g[i] = acc;
            cs[0] = cs[0] + a.x[i] * acc;
        }
    }
    ctl_block_sum<1>(cs, lds);
    if (tid == 0) a.part[blockIdx.x] = cs[0];
}

template <int L>
static void spq_launch_curv_L(hipStream_t st, const QnSpqArgs& a, const QnVecCtl* ctl) {
    hipLaunchKernelGGL(spq_curv_kernel<L>, dim3(a.G + a.n_long), dim3(SPQ_TPB), 0, st, a, ctl);
}

// enqueue one curvature pass of a sparse quadratic, with the lanes per row of the evaluation: q = Q d -> q_dev[0 .. n) and the shares (which & 1), then
// d'Qd -> c_dev by spq_finish_kernel (which & 2; the search adds the shares in exact_step_kernel instead, in the same order)
static int spq_enqueue_curvature(qn_objective* o, const double* d_dev, double* c_dev, double* q_dev, const QnVecCtl* ctl, int which, const QnObjWork*) {
    QnSpqArgs a{};
    a.row_ptr = o->sp.row_ptr; a.col = o->sp.col; a.val = o->sp.val; a.b = nullptr; a.wg_row_start = o->sp.wg_row_start; a.long_rows = o->sp.long_rows;
    a.x = d_dev; a.g = q_dev; a.part = o->sp.part;
    a.n = (int)o->n; a.G = o->sp.G; a.n_long = (int)o->sp.n_long;
    hipStream_t st = o->ctx->stream;
    if (which & 1) switch (o->sp.lanes) {
    case 1: spq_launch_curv_L<1>(st, a, ctl); break;
    case 2: spq_launch_curv_L<2>(st, a, ctl); break;
    case 4: spq_launch_curv_L<4>(st, a, ctl); break;
    case 8: spq_launch_curv_L<8>(st, a, ctl); break;
    case 16: spq_launch_curv_L<16>(st, a, ctl); break;
    case 32: spq_launch_curv_L<32>(st, a, ctl); break;
    case 64: spq_launch_curv_L<64>(st, a, ctl); break;
    default: return fail(QN_ERROR_INPUT_PARAMS, "sparse quadratic: lanes_per_row must be 1, 2, 4, 8, 16, 32 or 64");
    }
    if (which & 2) hipLaunchKernelGGL(spq_finish_kernel, dim3(1), dim3(SPQ_TPB), 0, st, a.part, a.G + a.n_long, c_dev);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

static void spq_curv_shares(const qn_objective* o, const double** part, int* count) { *part = o->sp.part; *count = o->sp.G + (int)o->sp.n_long; }
// qn_stats.obj_bytes: values + columns, the row offsets, and x, b, g of one evaluation; a curvature pass reads d, writes q and reads no b
static uint64_t spq_eval_bytes(const qn_objective* o) { return 12ull * (uint64_t)o->sp.nnz + 4ull * ((uint64_t)o->n + 1) + 24ull * (uint64_t)o->n; }
static uint64_t spq_curv_bytes(const qn_objective* o) { return 12ull * (uint64_t)o->sp.nnz + 4ull * ((uint64_t)o->n + 1) + 16ull * (uint64_t)o->n; }

static const QnObjOps kSpqOps = {
    /* eval */ spq_enqueue_eval, /* eval_launches */ 2, /* eval_split */ true, /* vec_counted */ true,
    /* weights */ nullptr, 0,
    /* hv_built, hess_vec, gbar, hv_out */ nullptr, nullptr, nullptr, nullptr, 0, false,
    /* curvature, curv_shares; hessian */ spq_enqueue_curvature, spq_curv_shares, nullptr, 0,
    /* bytes: eval, product, weights, curvature */ spq_eval_bytes, nullptr, nullptr, spq_curv_bytes,
    /* no_dense_family */ "unsupported objective",
    /* no_rows, no_hessian, no_curvature */ "a sparse quadratic has no dense rows / Hessian", "a sparse quadratic has no dense rows / Hessian", nullptr,
};
static const QnObjOps* spq_ops() { return &kSpqOps; }
