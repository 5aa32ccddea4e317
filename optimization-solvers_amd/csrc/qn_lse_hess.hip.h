// qn_lse_hess.hip.h -- the Hessian of the device log-sum-exp objective on the f64 matrix cores.
//
//   H(x) = A' diag(p) A - gbar gbar' + mu I,   p = softmax(A x + c),   gbar = A' p.
//
// p and gbar come from the launches of the two-pass evaluation (lse_enqueue_hessian, qn_host_objective.hip.h): z = A x, the
// single-workgroup softmax that leaves the NORMALISED weights in `wp.w` (zero past row m), the column sums and their fixed-order fold.
// What is new here is the one dense contraction the library lacked:
//
//   lse_hess_kernel<R, KC>   C = sum_k p_k a_k a_k' on the lower block triangle with v_mfma_f64_16x16x4_f64, then, in the same launch,
//                            H = C - gbar gbar' + mu I stored with its mirror image.
//
// A is row-major m x n_pad, so both operands of a C tile are K-MAJOR slabs: KC rows of A, T = 32 R consecutive columns each.  That is the
// transposed case of chol_syrk_kernel (which reads K-contiguous rows and turns them while staging): here a slab row goes to an LDS row
// as it lies in memory -- 16-byte loads coalesced along the columns, 16-byte LDS stores along the row: conflict-free.  The I operand is
// multiplied by p_k as it is staged (one v_mul per element, no pass of its own over A); the J operand is staged as it is.
// Fragment reads: lane l reads P[kk + (l >> 4)][w0 + (l & 15)] (A[i = l & 15][k = l >> 4] / B[k = l >> 4][j = l & 15]).  ds_read_b64 is
// served in two 32-lane halves over 64 banks of 4 bytes: a half holds two k rows of 16 consecutive doubles (32 banks each), so the rows
// must start 32 banks apart modulo 64 -- a row pitch of T + 16 doubles (80 / 144: 160 / 288 banks = 32 mod 64) makes the read
// conflict-free.  (chol_syrk_kernel's pitch of 65 leaves a 2-way conflict on 30 of 32 banks.)
// 256 threads = 4 waves, wave w owns the 16 R x 16 R quadrant (w >> 1, w & 1): R x R MFMA tiles.  The library carries ONE instance, R = 2:
// 64 x 64 per workgroup, KC = 32 -- the faster one at every size measured.  R = 4 (128 x 128 per workgroup, KC = 16; the two
// slabs of a chunk stay under the 64 KB of static LDS either way) exists for the measurement only: a diagnostic build with -DQN_LSE_HESS_TILE=128.
// The K loop is sequential and nothing is split across workgroups: every entry is ONE chain of fused multiply-adds in row order,
// so two calls at the same x give identical bits.
// Symmetry: an off-diagonal tile is stored twice, as it is and transposed.  On a diagonal tile C_ij and C_ji differ in the last bit
// (fl(p a_ki) a_kj against fl(p a_kj) a_ki), so only i >= j is taken from the accumulators and stored at (i, j) and (j, i):
// H == H' bit for bit by construction (gbar_i gbar_j is one rounded product either way, -ffp-contract=off).
// Tails: rows k >= m and columns >= n_pad are staged as zeros (neither A nor p is read there); entries outside n_pad x n_pad are not stored.
#pragma once

#ifndef QN_LSE_HESS_TILE
#define QN_LSE_HESS_TILE 64
#endif
static_assert(QN_LSE_HESS_TILE == 64 || QN_LSE_HESS_TILE == 128, "QN_LSE_HESS_TILE is 64 or 128");

template <int R, int KC>
__global__ __launch_bounds__(256) void lse_hess_kernel(const double* __restrict__ A, const double* __restrict__ p, const double* __restrict__ gbar,
                                                       double mu, int m, int np, int ntiles, double* __restrict__ H, size_t ld) {
    constexpr int T = 32 * R;        // tile edge
    constexpr int W = 16 * R;        // a wave's quadrant edge
    constexpr int PITCH = T + 16;    // doubles per LDS row (see above)
    constexpr int CP = T / 2;        // column pairs per slab row
    constexpr int RSTEP = 256 / CP;  // slab rows staged per sweep of the workgroup
    constexpr int NU = KC / RSTEP;   // sweeps per chunk
    static_assert(KC % RSTEP == 0 && KC % 4 == 0, "chunk depth");
    __shared__ __attribute__((aligned(16))) double PI[KC][PITCH]; // PI[k][i] = p_k A[k][i0 + i]
    __shared__ __attribute__((aligned(16))) double PJ[KC][PITCH]; // PJ[k][j] =     A[k][j0 + j]
    int ti, tj;
    qn_tri_tile(blockIdx.x, ntiles, ti, tj);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = ti * T, j0 = tj * T;
    const int wi = (wave >> 1) * W, wj = (wave & 1) * W;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int sc = 2 * (tid % CP), sr = tid / CP; // this thread's column pair and first slab row
    const bool ci_ok = i0 + sc < np, cj_ok = j0 + sc < np; // (n_pad is even: a pair is inside or outside as a whole)
    const double* ai = A + (size_t)i0 + sc;
    const double* aj = A + (size_t)j0 + sc;
    v2d vi[NU], vj[NU];
    double pw[NU];
    auto load_chunk = [&](int k0) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int k = k0 + sr + RSTEP * u;
            const bool k_ok = k < m;
            pw[u] = k_ok ? p[k] : 0.0;
            vi[u] = (k_ok && ci_ok) ? ld2(ai + (size_t)k * np) : (v2d){0.0, 0.0};
            vj[u] = (k_ok && cj_ok) ? ld2(aj + (size_t)k * np) : (v2d){0.0, 0.0};
        }
    };
    load_chunk(0);
    v4d acc[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) acc[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < m; k0 += KC) {
        if (k0) __syncthreads();
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int kr = sr + RSTEP * u;
            v2d s;
            s.x = pw[u] * vi[u].x;
            s.y = pw[u] * vi[u].y;
            *reinterpret_cast<v2d*>(&PI[kr][sc]) = s;
            *reinterpret_cast<v2d*>(&PJ[kr][sc]) = vj[u];
        }
        __syncthreads();
        if (k0 + KC < m) load_chunk(k0 + KC); // the next chunk's loads fly while this one is multiplied
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            double fa[R], fb[R];
#pragma unroll
            for (int a = 0; a < R; ++a) { fa[a] = PI[kk + l4][wi + 16 * a + l15]; fb[a] = PJ[kk + l4][wj + 16 * a + l15]; }
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int b = 0; b < R; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
    }
    // epilogue: H = C - gbar gbar' + mu I, the tile and its mirror image
    const bool diag_tile = ti == tj;
#pragma unroll
    for (int b = 0; b < R; ++b) {
        const int j = j0 + wj + 16 * b + l15;
        if (j >= np) continue;
        const double gj = gbar[j];
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) { // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
                const int i = i0 + wi + 16 * a + l4 + 4 * reg;
                if (i >= np || (diag_tile && j > i)) continue;
                const double gg = gbar[i] * gj;
                double h = acc[a][b][reg] - gg;
                if (i == j) h = h + mu;
                H[(size_t)i * ld + j] = h;
                if (i != j) H[(size_t)j * ld + i] = h;
            }
    }
}

static int lse_hess_launch(hipStream_t st, const double* A, const double* p, const double* gbar, double mu, int m, int np, double* H, size_t ld) {
    constexpr int R = QN_LSE_HESS_TILE / 32, KC = QN_LSE_HESS_TILE == 64 ? 32 : 16;
    const int nt = (np + QN_LSE_HESS_TILE - 1) / QN_LSE_HESS_TILE;
    hipLaunchKernelGGL((lse_hess_kernel<R, KC>), dim3((unsigned)qn_tri_tiles(nt, nt)), dim3(256), 0, st, A, p, gbar, mu, m, np, nt, H, ld);
    HIPCHK(hipGetLastError());
    return QN_OK;
}
