// qn_rank1.hip.h -- Broyden / BroydenB (quasi_newton/broyden.rs, broyden_b.rs): the one solver of the dense quasi-Newton family whose inverse
// Hessian is NOT symmetric after its first update, and whose update needs a COLUMN product:
//
//     hy = H y ;  H += ((s - hy) s') H / (s.y)          (broyden.rs:115-118)
//         = H + c a w' ,   a = s - H y ,  w = H' s ,  c = 1 / (s.y)
//
// (w is a row vector times H: it equals H s only while H is symmetric, i.e. for the very first update.  The denominator is s.y as written,
// not s'Hy: this is not the textbook formula and H+ y = s does not hold.)  None of the symmetric-storage kernels can hold such an H, and no
// other kernel here sums columns -- hence this file.  Included by qn_kernels.hip.h in front of the control step.
//
//   r1_pass_kernel    one workgroup per 128 x 128 tile of the full row-major H (ragged at the edge: n_pad is a multiple of 16, not of 128).
//                     Applies the PENDING update H_stored + c a w' and writes the tile back (padding stays exactly zero), and from the same
//                     registers forms the tile's ROW partials against up to two right-hand sides (u = H y, v = H g+) and its COLUMN
//                     partials against s (w = H' s).  A wave owns 32 rows, a lane two adjacent columns (one 16-byte access per row, a wave
//                     instruction = one whole tile row of 1 KiB); eight rows are in flight per trip.  Row partials: a halving butterfly over
//                     the wave (32 values per right-hand side -> 32 shuffles each).  Column partials: per-lane accumulators, the four waves
//                     added through LDS in wave order.  16 n^2 algorithmic bytes with a pending update, like the generic BFGS pass.
//   r1_reduce_kernel  the second stage: row partials [nrhs][nb][n_pad] summed over the tile COLUMNS in ascending order into the generic path's
//                     gathered buffer (V.hp: u at [0, n_pad), v at [n_pad, 2 n_pad)), column partials [nb][n_pad] over the tile ROWS into
//                     `up` -- the new w; the pass has finished with the old one.
// No floating-point atomics: every sum has a fixed order, two identical runs give the same bits.
// (n <= QN_SMALL_N never comes here: small_update has the reference's literal triple product.)
#pragma once

#define QN_R1_TB 128        // tile side
#define QN_R1_WIN 8         // rows in flight per wave

struct QnR1Args {
    double* H;
    int n, n_pad, nb;     // nb = ceil(n_pad / QN_R1_TB) tiles per side
    const double *a, *w;  // the pending update's vectors (QnVecs.sp, QnVecs.up)
    double c;             // ... and its coefficient (QnCtl.c_ss)
    const double *r0, *r1; // right-hand sides of the row sums
    const double* scol;   // left-hand side of the column sums
    double* rowpart;      // [2][nb][n_pad]
    double* colpart;      // [nb][n_pad]
    double* hp;           // reduce: row totals, [2][n_pad]
    double* wout;         // reduce: column totals
    int nrhs, col;
};

// lane k's value in every lane (k is a compile-time constant once the loops are unrolled: two v_readlane_b32)
__device__ __forceinline__ double qn_r1_bcast(const double v, const int k) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

template <int WIN, int NRHS, bool PENDING, bool COL>
struct QnR1Window {
    static __device__ __forceinline__ void run(const QnR1Args& a, const int row0, const int jc, const bool jin, const bool c0, const bool c1,
                                               const v2d wj, const v2d y0, const v2d y1, const double al, const double sl,
                                               double (&acc0)[32], double (&acc1)[32], v2d& cacc) {
        constexpr int W0 = WIN * QN_R1_WIN;
        const int np = a.n_pad;
        v2d h[QN_R1_WIN];
#pragma unroll
        for (int r = 0; r < QN_R1_WIN; ++r) {
            const int i = row0 + W0 + r;
            h[r] = ld2(a.H + (size_t)(i < np ? i : 0) * (size_t)np + jc); // (rows past the edge: a harmless re-read of row 0, masked below)
        }
#pragma unroll
        for (int r = 0; r < QN_R1_WIN; ++r) {
            const int i = row0 + W0 + r;
            const bool in = i < np && jin;
            v2d hn = h[r];
            if (PENDING) {
                const double ai = qn_r1_bcast(al, W0 + r);
                hn.x = hn.x + a.c * (ai * wj.x);
                hn.y = hn.y + a.c * (ai * wj.y);
                hn.x = (i < a.n && c0) ? hn.x : 0.0; // padding stays exactly zero
                hn.y = (i < a.n && c1) ? hn.y : 0.0;
                if (in) st2(a.H + (size_t)i * (size_t)np + jc, hn);
            }
            if (!in) hn = (v2d){0.0, 0.0};
            if (NRHS >= 1) acc0[W0 + r] = __builtin_fma(hn.y, y0.y, hn.x * y0.x);
            if (NRHS >= 2) acc1[W0 + r] = __builtin_fma(hn.y, y1.y, hn.x * y1.x);
            if (COL) {
                const double si = qn_r1_bcast(sl, W0 + r);
                cacc.x = __builtin_fma(hn.x, si, cacc.x);
                cacc.y = __builtin_fma(hn.y, si, cacc.y);
            }
        }
    }
};

template <int NRHS, bool PENDING, bool COL>
__global__ __launch_bounds__(256) void r1_pass_kernel(const QnR1Args a) {
    __shared__ double colred[4][QN_R1_TB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int I = blockIdx.y, J = blockIdx.x;
    const int np = a.n_pad;
    const int j = J * QN_R1_TB + 2 * lane; // this lane's column pair (n_pad and j are even: both columns are inside, or neither)
    const bool jin = j < np;
    const int jc = jin ? j : 0;
    const bool c0 = j < a.n, c1 = j + 1 < a.n;
    const int row0 = I * QN_R1_TB + wave * 32;
    v2d wj = {0.0, 0.0}, y0 = {0.0, 0.0}, y1 = {0.0, 0.0};
    if (PENDING) wj = ld2(a.w + jc);
    if (NRHS >= 1) y0 = ld2(a.r0 + jc);
    if (NRHS >= 2) y1 = ld2(a.r1 + jc);
    // the wave's 32 entries of a and s: lane l holds row row0 + l, broadcast by v_readlane where they are used
    double al = 0.0, sl = 0.0;
    {
        const int i = row0 + (lane & 31);
        const int ic = i < np ? i : 0;
        if (PENDING) al = a.a[ic];
        if (COL) sl = a.scol[ic];
    }
    double acc0[32], acc1[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) { acc0[k] = 0.0; acc1[k] = 0.0; }
    v2d cacc = {0.0, 0.0};
    QnR1Window<0, NRHS, PENDING, COL>::run(a, row0, jc, jin, c0, c1, wj, y0, y1, al, sl, acc0, acc1, cacc);
    QnR1Window<1, NRHS, PENDING, COL>::run(a, row0, jc, jin, c0, c1, wj, y0, y1, al, sl, acc0, acc1, cacc);
    QnR1Window<2, NRHS, PENDING, COL>::run(a, row0, jc, jin, c0, c1, wj, y0, y1, al, sl, acc0, acc1, cacc);
    QnR1Window<3, NRHS, PENDING, COL>::run(a, row0, jc, jin, c0, c1, wj, y0, y1, al, sl, acc0, acc1, cacc);
    // row partials: the wave's 64 lanes hold the 128 columns of each of its 32 rows; after the fold lane l has row (l >> 1) in [0]
    if (NRHS >= 1) {
        QnWaveFold<32, 32>::run(acc0, lane);
        const int i = row0 + (lane >> 1);
        if ((lane & 1) == 0 && i < np) a.rowpart[(size_t)J * (size_t)np + i] = acc0[0];
    }
    if (NRHS >= 2) {
        QnWaveFold<32, 32>::run(acc1, lane);
        const int i = row0 + (lane >> 1);
        if ((lane & 1) == 0 && i < np) a.rowpart[((size_t)a.nb + J) * (size_t)np + i] = acc1[0];
    }
    if (COL) { // column partials: the four waves' 32-row shares, added in wave order
        colred[wave][2 * lane] = cacc.x;
        colred[wave][2 * lane + 1] = cacc.y;
        __syncthreads();
        const int jj = J * QN_R1_TB + tid;
        if (tid < QN_R1_TB && jj < np) a.colpart[(size_t)I * (size_t)np + jj] = ((colred[0][tid] + colred[1][tid]) + colred[2][tid]) + colred[3][tid];
    }
}

__global__ __launch_bounds__(256) void r1_reduce_kernel(const QnR1Args a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int np = a.n_pad;
    if (i >= np) return;
    for (int rhs = 0; rhs < a.nrhs; ++rhs) {
        const double* p = a.rowpart + (size_t)rhs * a.nb * (size_t)np + i;
        double t = p[0];
        for (int J = 1; J < a.nb; ++J) t = t + p[(size_t)J * np];
        a.hp[(size_t)rhs * np + i] = t;
    }
    if (a.col) {
        const double* p = a.colpart + i;
        double t = p[0];
        for (int I = 1; I < a.nb; ++I) t = t + p[(size_t)I * np];
        a.wout[i] = t;
    }
}
