// qn_sparse_multinomial.hip.h -- the sparse softmax-regression objective (OBJ_SPARSE_MULTINOMIAL): Multinomial's function (qn_multinomial.hip.h) on a
// CSR A (m x n, one rank), labels in {0, .., K-1}, sample weights w_i >= 0, ridge mu.  The parameter vector is CLASS-MAJOR, x[k n + j] = W[k, j],
// N = K n entries; g and H v have the same layout.  No limit on K n, none on K (m K and K n index with 32 bits).
//
// Both halves of an evaluation are a sparse matrix times a skinny dense one, Z = A Wt (m x n times n x K) and Gt = A' C (n x m times m x K).  As in
// the sparse logistic objective the device holds A AND A' (24 bytes per nonzero), the transpose product walks the rows of A' with the code that walks
// the rows of A, and no float atomic is used.  The skinny matrices are FEATURE-MAJOR / ROW-MAJOR with the padded leading dimension Kp (smn_kp: the
// next power of two up to 16, a multiple of 16 above -- a row of K doubles never straddles a 128-byte line it need not), so that the K values one
// nonzero multiplies are contiguous.  FIVE launches per evaluation and per product:
//
//   smn_in_kernel                  Wt[j Kp + k] = x[k n + j] (or v) through a TK x TJ tile in LDS (TK = min(Kp, 32), TK TJ = 1024); k >= K: zeros
//   smn_rows_kernel<PRODUCT, ONE>  a row is owned by L x CL consecutive lanes of a wave (lane = l CL + cl): CL class lanes (smn_cl: the next power of
//                                  two of K, at most 64 / L), L entry lanes.  Classes go by in CLASS BLOCKS of CL x SMN_KR: slot r of class lane cl
//                                  in block b is the class k = (b SMN_KR + r) CL + cl.  Per block, entry lane l adds the products a_ij Wt[j Kp + k] of
//                                  entries l, l + L, .. in that order (one load of the value and the column feeds SMN_KR products; the CL lanes read
//                                  contiguous doubles), then the xor tree L CL / 2 .. CL over the entry lanes.  ONE (K <= CL SMN_KR: one block): the
//                                  margins stay in registers.  Otherwise the margins of a block are PARKED in the row's slice of the coefficient
//                                  buffer (the lane that stores a value is the lane that reads it back) until the last block is done.
//                                  A row of more than SPQ_LONG_ROW entries is summed by workgroup G + k of the same launch: 256 / CLw entry lanes
//                                  (CLw = smn_cl at L = 1), the xor tree 32 .. CLw inside a wave, the four waves' partial sums added in WAVE ORDER.
//                                  THE RULES PER ROW (those of qn_multinomial.hip.h; entry lane 0's class lanes work, a lane's classes in ascending
//                                  order, then the xor tree CL / 2 .. 1 over the class lanes -- THE ORDER OF S, Sn AND ubar: fixed by (K, L)):
//                                    evaluation  zmax = max_k z_k (the row's own); e_k = exp(z_k - zmax); S = sum e_k; Sn = sum_{k != y} e_k;
//                                                p_k = e_k / S (IEEE division); l = (zmax - z_y) + log(S); c_k = w p_k (k != y), c_y = -(w (Sn / S))
//                                                -- never w (p_y - 1); w = 0: l = 0, c_k = 0 and P_k = 0 BY SELECTS.  C and P (m x Kp) are stored, the
//                                                row's w l is added to the lane's sum (rows in index order), the workgroup leaves ONE share of the loss
//                                    product     z = u = A Vt; p_k from the stored P; ubar = sum_k p_k u_k (product and sum round separately);
//                                                t_k = (w p_k)(u_k - ubar), w = 0: 0 by a select; T (m x Kp) is stored; no transcendental function
//   smn_cols_kernel                the same geometry over the rows of A' (the columns of A), gathering C or T: Gt[j Kp + k] = sum_i a_ij c_ik
//   smn_out_kernel                 back to class-major through the same LDS tile: g[k n + j] = Gt[j Kp + k] + mu x[k n + j] and the workgroup's share
//                                  of sum x^2 (evaluation) or of sum v q (product); mu x rounds on its own, x^2 and v q before they are added.
//                                  Entries N .. N_pad are never written.  Its grid is a function of (n, Kp) alone: at most SMN_TGRID shares
//   slog_finish_kernel             (qn_sparse_logistic.hip.h, as it stands) f = sum(loss shares) + 0.5 mu sum(xx shares); in product mode the shares of
//                                  v'Hv folded into ONE value, which NewtonCG reads with kcount = 1
//
// No atomics, no workgroup waits for another, every order is fixed by (pattern, K, L): the same bits from run to run, from object to object and for
// int32 and int64 index arrays.  Products and sums round separately (-ffp-contract=off).  Product launches take `ctl` and return at once unless
// NewtonCG's inner loop is running (slog_skip); null: they always run.
//
// ADDRESSING: 32-bit element indices into the CSR arrays (nnz <= 2^31 - 1, m, n <= 2^30), 64-bit offsets into the skinny matrices (rows Kp).  Nothing
// is read past row_ptr[rows]; columns were checked against the other dimension on the host; every class index is compared with K before it is used;
// a tile of the two transposing kernels compares j with n and k with K (Kp).
#pragma once

#define SMN_KR 4       // class slots per lane and class block
#define SMN_TGRID 1024 // workgroups of the two transposing launches at the most

struct QnSmnArgs {
    const int* row_ptr;      // rows + 1 of the copy this launch walks
    const int* col;          // nnz
    const double* val;       // nnz
    const int* wg_row_start; // G + 1
    const int* long_rows;    // n_long
    const double* src;       // the gathered skinny matrix, leading dimension Kp: Wt / Vt (row pass), C / T (column pass)
    double* out;             // row pass: C (evaluation: the margins are parked here) or T; column pass: Gt
    double* P;               // row pass: evaluation stores it (and parks e in it), the product reads it (m x Kp)
    const double* wt;        // row pass: the sample weights (m)
    const int* lab;          // row pass: the labels (m)
    double* part;            // row pass, evaluation: G + n_long shares of the loss
    int G, n_long, K, Kp, L, CL, CLw;
};

__host__ __device__ __forceinline__ int smn_pow2_ceil(int k) { int p = 1; while (p < k) p *= 2; return p; }
// the padded leading dimension: rests on the one measurement there is (full load rate for contiguous segments of 128 bytes and above, 64 lanes in 64
// rows about 17 times slower; 8 to 64 bytes unmeasured): a small K is padded to a power of two so that no row of K doubles crosses a 128-byte line
__host__ __device__ __forceinline__ int smn_kp(int K) { return K <= 16 ? (K < 2 ? 2 : smn_pow2_ceil(K)) : (K + 15) / 16 * 16; }
// class lanes beside L entry lanes
__host__ __device__ __forceinline__ int smn_cl(int K, int L) { const int c = smn_pow2_ceil(K < 64 ? K : 64), cap = 64 / L; return c < cap ? c : cap; }

// what the class lanes of a row do with its margins.  Slot r of block b is class (b SMN_KR + r) CL + cl; ONE: z[] holds block 0 (the only one),
// otherwise the margins are read back from a.out.  `active`: this lane stores (entry lane 0 of a row that exists); every lane of the wave runs the
// shuffles.  Returns the row's loss term w l (evaluation, on the active lanes; the same bits in every class lane)
template <bool PRODUCT, bool ONE>
__device__ __forceinline__ double smn_row_end(const QnSmnArgs& a, int i, int cl, int CL, bool active, const double (&z)[SMN_KR]) {
    const int K = a.K, nb = ONE ? 1 : (K + CL * SMN_KR - 1) / (CL * SMN_KR);
    const size_t base = (size_t)i * (size_t)a.Kp;
    const double w = active ? a.wt[i] : 0.0;
    const bool live = w != 0.0;
    if (PRODUCT) {
        double ubar = 0.0, p1[SMN_KR];
        for (int b = 0; b < nb; ++b)
#pragma unroll
            for (int r = 0; r < SMN_KR; ++r) {
                const int k = (b * SMN_KR + r) * CL + cl;
                const bool in = active && k < K;
                const double p = in ? a.P[base + k] : 0.0;
                const double u = ONE ? z[r] : (in ? a.out[base + k] : 0.0);
                if (ONE) p1[r] = p;
                ubar = ubar + (in ? p * u : 0.0);
            }
        for (int off = CL / 2; off >= 1; off >>= 1) ubar = ubar + __shfl_xor(ubar, off, 64);
        for (int b = 0; b < nb; ++b)
#pragma unroll
            for (int r = 0; r < SMN_KR; ++r) {
                const int k = (b * SMN_KR + r) * CL + cl;
                if (active && k < K) {
                    const double p = ONE ? p1[r] : a.P[base + k];
                    const double u = ONE ? z[r] : a.out[base + k];
                    const double t = (w * p) * (u - ubar);
                    a.out[base + k] = live ? t : 0.0;
                }
            }
        return 0.0;
    }
    const int y = active ? a.lab[i] : 0;
    double zmax = -INFINITY, zy = 0.0;
    for (int b = 0; b < nb; ++b)
#pragma unroll
        for (int r = 0; r < SMN_KR; ++r) {
            const int k = (b * SMN_KR + r) * CL + cl;
            if (active && k < K) {
                const double zz = ONE ? z[r] : a.out[base + k];
                zmax = fmax(zmax, zz);
                if (k == y) zy = zz;
            }
        }
    for (int off = CL / 2; off >= 1; off >>= 1) {
        zmax = fmax(zmax, __shfl_xor(zmax, off, 64));
        zy = zy + __shfl_xor(zy, off, 64); // (one lane holds z_y, the others 0.0)
    }
    double S = 0.0, Sn = 0.0, e1[SMN_KR];
    for (int b = 0; b < nb; ++b)
#pragma unroll
        for (int r = 0; r < SMN_KR; ++r) {
            const int k = (b * SMN_KR + r) * CL + cl;
            const bool in = active && k < K;
            const double e = in ? exp((ONE ? z[r] : a.out[base + k]) - zmax) : 0.0;
            if (ONE) e1[r] = e;
            else if (in) a.P[base + k] = e; // (parked: read back below by this lane)
            S = S + e;
            Sn = Sn + (k == y ? 0.0 : e);
        }
    for (int off = CL / 2; off >= 1; off >>= 1) {
        S = S + __shfl_xor(S, off, 64);
        Sn = Sn + __shfl_xor(Sn, off, 64);
    }
    const double cy = -(w * (Sn / S));
    for (int b = 0; b < nb; ++b)
#pragma unroll
        for (int r = 0; r < SMN_KR; ++r) {
            const int k = (b * SMN_KR + r) * CL + cl;
            if (active && k < K) {
                const double p = (ONE ? e1[r] : a.P[base + k]) / S;
                a.out[base + k] = live ? (k == y ? cy : w * p) : 0.0;
                a.P[base + k] = live ? p : 0.0;
            }
        }
    const double l = (zmax - zy) + log(S);
    return live ? w * l : 0.0;
}

// ROWS: the row pass (with smn_row_end) or, false, the column pass (the sums are stored as they are)
template <bool ROWS, bool PRODUCT, bool ONE>
__device__ __forceinline__ void smn_pass(const QnSmnArgs& a, double* lds) {
    const int tid = threadIdx.x, K = a.K, Kp = a.Kp;
    double fs[1] = {0.0};
    if ((int)blockIdx.x >= a.G) { // one long row, the whole workgroup: 256 / CLw entry lanes, the waves added in wave order
        const int i = a.long_rows[blockIdx.x - a.G];
        const int CL = a.CLw, LE = SPQ_TPB / CL, e = tid / CL, cl = tid % CL, wave = tid >> 6;
        const int j0 = a.row_ptr[i], j1 = a.row_ptr[i + 1];
        const int nb = (K + CL * SMN_KR - 1) / (CL * SMN_KR);
        const bool active = tid < CL;
        const size_t base = (size_t)i * (size_t)Kp;
        double* wl = lds + 16; // [4 waves][CL][SMN_KR]
        double z[SMN_KR] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < nb; ++b) {
            double acc[SMN_KR];
#pragma unroll
            for (int r = 0; r < SMN_KR; ++r) acc[r] = 0.0;
            for (int j = j0 + e; j < j1; j += LE) {
                const double av = a.val[j];
                const double* s = a.src + (size_t)a.col[j] * (size_t)Kp;
#pragma unroll
                for (int r = 0; r < SMN_KR; ++r) {
                    const int k = (b * SMN_KR + r) * CL + cl;
                    if (k < K) acc[r] = acc[r] + av * s[k];
                }
            }
            for (int off = 32; off >= CL; off >>= 1)
#pragma unroll
                for (int r = 0; r < SMN_KR; ++r) acc[r] = acc[r] + __shfl_xor(acc[r], off, 64);
            if ((tid & 63) < CL)
#pragma unroll
                for (int r = 0; r < SMN_KR; ++r) wl[(wave * CL + cl) * SMN_KR + r] = acc[r];
            __syncthreads();
            if (active)
#pragma unroll
                for (int r = 0; r < SMN_KR; ++r) {
                    double t = wl[cl * SMN_KR + r];
                    for (int wv = 1; wv < SPQ_TPB / 64; ++wv) t = t + wl[(wv * CL + cl) * SMN_KR + r];
                    z[r] = t;
                    const int k = (b * SMN_KR + r) * CL + cl;
                    if ((!ROWS || !ONE) && k < K) a.out[base + k] = t;
                }
            __syncthreads();
        }
        if (ROWS && tid < 64) { // (wave 0: its first CL lanes hold the row)
            const double term = smn_row_end<PRODUCT, ONE>(a, i, cl, CL, active, z);
            if (!PRODUCT && tid == 0) a.part[blockIdx.x] = term;
        }
        return;
    }
    const int L = a.L, CL = a.CL, GL = L * CL, RPT = SPQ_TPB / GL; // rows per trip
    const int r0 = a.wg_row_start[blockIdx.x], r1 = a.wg_row_start[blockIdx.x + 1];
    const int sub = tid / GL, g = tid % GL, l = g / CL, cl = g % CL;
    const int nb = ONE ? 1 : (K + CL * SMN_KR - 1) / (CL * SMN_KR);
    for (int rb = r0; rb < r1; rb += RPT) {
        const int i = rb + sub;
        int j0 = 0, j1 = 0;
        if (i < r1) { j0 = a.row_ptr[i]; j1 = a.row_ptr[i + 1]; }
        const bool regular = j1 - j0 <= SPQ_LONG_ROW; // (a long row: nothing here, its own workgroup stores its results and its share)
        const bool active = l == 0 && i < r1 && regular;
        const size_t base = (size_t)i * (size_t)Kp;
        double z[SMN_KR];
        for (int b = 0; b < nb; ++b) {
#pragma unroll
            for (int r = 0; r < SMN_KR; ++r) z[r] = 0.0;
            if (regular)
                for (int j = j0 + l; j < j1; j += L) {
                    const double av = a.val[j];
                    const double* s = a.src + (size_t)a.col[j] * (size_t)Kp;
#pragma unroll
                    for (int r = 0; r < SMN_KR; ++r) {
                        const int k = (b * SMN_KR + r) * CL + cl;
                        if (k < K) z[r] = z[r] + av * s[k];
                    }
                }
            for (int off = GL / 2; off >= CL; off >>= 1)
#pragma unroll
                for (int r = 0; r < SMN_KR; ++r) z[r] = z[r] + __shfl_xor(z[r], off, 64);
            if ((!ROWS || !ONE) && active)
#pragma unroll
                for (int r = 0; r < SMN_KR; ++r) {
                    const int k = (b * SMN_KR + r) * CL + cl;
                    if (k < K) a.out[base + k] = z[r];
                }
        }
        if (ROWS) {
            const double term = smn_row_end<PRODUCT, ONE>(a, i, cl, CL, active, z);
            if (active && cl == 0) fs[0] = fs[0] + term;
        }
    }
    if (ROWS && !PRODUCT) {
        ctl_block_sum<1>(fs, lds);
        if (tid == 0) a.part[blockIdx.x] = fs[0];
    }
}

template <bool PRODUCT, bool ONE>
__global__ __launch_bounds__(SPQ_TPB) void smn_rows_kernel(const QnSmnArgs a, const QnVecCtl* ctl) {
    __shared__ double lds[16 + SPQ_TPB * SMN_KR];
    if (PRODUCT && slog_skip(ctl)) return;
    smn_pass<true, PRODUCT, ONE>(a, lds);
}

__global__ __launch_bounds__(SPQ_TPB) void smn_cols_kernel(const QnSmnArgs a, const QnVecCtl* ctl, int product) {
    __shared__ double lds[16 + SPQ_TPB * SMN_KR];
    if (product && slog_skip(ctl)) return;
    smn_pass<false, false, false>(a, lds);
}

// the tiles of the two transposing launches: TK = min(Kp, 32) classes x TJ = 1024 / TK features, tile t = (t / tiles_k) features, (t % tiles_k) classes
struct QnSmnTile { int n, K, Kp, TK, TJ, tiles_k, tiles; };

// Wt[j Kp + k] = x[k n + j], zeros for K <= k < Kp
__global__ __launch_bounds__(SPQ_TPB) void smn_in_kernel(const QnSmnTile t, const double* x, double* wt, const QnVecCtl* ctl, int product) {
    __shared__ double tile[1024 + 32];
    if (product && slog_skip(ctl)) return;
    const int tid = threadIdx.x, TJ = t.TJ, TK = t.TK;
    for (int tt = blockIdx.x; tt < t.tiles; tt += gridDim.x) {
        const int j0 = (tt / t.tiles_k) * TJ, k0 = (tt % t.tiles_k) * TK;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = tid + SPQ_TPB * e, jj = idx % TJ, kk = idx / TJ;
            const int j = j0 + jj, k = k0 + kk;
            tile[kk * (TJ + 1) + jj] = (j < t.n && k < t.K) ? x[(size_t)k * (size_t)t.n + j] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = tid + SPQ_TPB * e, kk = idx % TK, jj = idx / TK;
            const int j = j0 + jj, k = k0 + kk;
            if (j < t.n && k < t.Kp) wt[(size_t)j * (size_t)t.Kp + k] = tile[kk * (TJ + 1) + jj];
        }
        __syncthreads();
    }
}

// g[k n + j] = Gt[j Kp + k] + mu xv[k n + j]; part[workgroup] = the share of sum xv^2 (product == 0) or sum xv g (product != 0): a thread adds
// its entries in tile order, then the block sum
__global__ __launch_bounds__(SPQ_TPB) void smn_out_kernel(const QnSmnTile t, const double* gt, const double* xv, double mu, double* g, double* part,
                                                          const QnVecCtl* ctl, int product) {
    __shared__ double tile[1024 + 32];
    __shared__ double lds[16];
    if (product && slog_skip(ctl)) return;
    const int tid = threadIdx.x, TJ = t.TJ, TK = t.TK;
    double fs[1] = {0.0};
    for (int tt = blockIdx.x; tt < t.tiles; tt += gridDim.x) {
        const int j0 = (tt / t.tiles_k) * TJ, k0 = (tt % t.tiles_k) * TK;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = tid + SPQ_TPB * e, kk = idx % TK, jj = idx / TK;
            const int j = j0 + jj, k = k0 + kk;
            tile[kk * (TJ + 1) + jj] = (j < t.n && k < t.K) ? gt[(size_t)j * (size_t)t.Kp + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = tid + SPQ_TPB * e, jj = idx % TJ, kk = idx / TJ;
            const int j = j0 + jj, k = k0 + kk;
            if (j < t.n && k < t.K) {
                const size_t at = (size_t)k * (size_t)t.n + j;
                const double xj = xv[at];
                const double mx = mu * xj;
                const double gj = tile[kk * (TJ + 1) + jj] + mx;
                g[at] = gj;
                const double term = product ? xj * gj : xj * xj;
                fs[0] = fs[0] + term;
            }
        }
        __syncthreads();
    }
    ctl_block_sum<1>(fs, lds);
    if (tid == 0) part[blockIdx.x] = fs[0];
}

static QnSmnTile smn_tile(int n, int K, int Kp) {
    QnSmnTile t{};
    t.n = n; t.K = K; t.Kp = Kp; t.TK = Kp < 32 ? Kp : 32; t.TJ = 1024 / t.TK;
    t.tiles_k = (Kp + t.TK - 1) / t.TK;
    const long long tiles = (long long)((n + t.TJ - 1) / t.TJ) * t.tiles_k; // (n <= 2^30, Kp n < 2^32: far inside an int)
    t.tiles = (int)tiles;
    return t;
}
static int smn_tile_grid(const QnSmnTile& t) { return t.tiles < SMN_TGRID ? t.tiles : SMN_TGRID; }

// the row pass: ONE where the class lanes' SMN_KR slots hold all K classes
template <bool PRODUCT>
static void smn_launch_rows(hipStream_t st, const QnSmnArgs& a, const QnVecCtl* ctl) {
    if (a.K <= a.CL * SMN_KR) hipLaunchKernelGGL((smn_rows_kernel<PRODUCT, true>), dim3(a.G + a.n_long), dim3(SPQ_TPB), 0, st, a, ctl);
    else hipLaunchKernelGGL((smn_rows_kernel<PRODUCT, false>), dim3(a.G + a.n_long), dim3(SPQ_TPB), 0, st, a, ctl);
}
