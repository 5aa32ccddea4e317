// qn_pnorm.hip.h -- the direction kernels of the two steepest-descent solvers whose direction does not come out of the control kernel's own sweep:
//
//   PnormDescent      (steepest_descent/pnorm_descent.rs:35)        d = (-inverse_p) * g, inverse_p a caller's dense n x n matrix that never changes
//   CoordinateDescent (steepest_descent/coordinate_descent.rs:30-44) d = -e_p, p the FIRST index of the largest |g_i| (strict >, NaN never wins)
//
// Included by qn_kernels.hip.h in front of the control step, whose QN_ST_AFTER_STEEP consumes what these kernels leave (QnVecs.steep_part).
//
//   pnorm_dir_kernel<RW, NT>   ONE launch per iteration, ONE read-only stream of the matrix (8 n_pad^2 bytes, row-major, padded with zeros as H is).
//       A workgroup is 4 waves, a wave owns RW rows and sweeps ALL their columns itself: per step a lane loads 16 bytes of each of its RW rows (one
//       wave instruction = 1 KiB of one row), RW x U loads in flight per lane (RW = 2: U = 4, RW = 4: U = 2).  g is staged in LDS in chunks of
//       QN_PN_CH = 4096 columns (32 KiB -- at n = 32768 all of g is 256 KiB and does not fit a CU's 160 KiB, so the chunk loop is not an option) and read
//       from there once per step for all RW rows.  Row sums: one accumulator per lane and row, then the halving butterfly over the wave.
//       The row's owner has d_i and g_i in hand, so the same launch leaves, per QN_PN_SHARE rows, the shares of g.d, ||g||_inf and the count of
//       non-finite d_i: the line search's first decision needs no further pass over a vector.
//       SUMMATION ORDER, fixed by n alone: lane l of the row's wave adds columns 2l, 2l+1, 2l+128, 2l+129, ... in ascending order, then the lanes are
//       added xor 32, 16, 8, 4, 2, 1; a share adds its rows in ascending order.  Neither depends on RW, on NT or on the grid: every instance gives
//       the same bits (tested), and two runs repeat bit for bit -- no float atomics, no waiting between workgroups.
//       FMA: the build is -ffp-contract=off; the column accumulations and the share's g_i d_i accumulation ASK for an FMA (__builtin_fma, one rounding
//       per term) -- n > 5 is tolerance-level parity with the reference's two-rounding column sweep (tests/steepest_cases.py).  d_i = -(sum): an exact
//       negation, so (-P) g and -(P g) have the same bits and the matrix is kept as given.
//       Grid: n_pad / (4 RW) workgroups (n_pad is a multiple of 16: every row of every workgroup exists).  Columns and rows >= n are masked by
//       selects, so the padding stays out of every sum whatever it holds.
//       NT: the matrix through non-temporal loads.  It is read once per iteration and nothing else reads it; whether passing the caches by pays is a
//       measurement (tools/bench_pnorm.py): the host side picks by size, QN_OPT_PNORM_NONTEMPORAL overrides.
//   cd_argmax_kernel           stage one of the (magnitude, index) reduction: G = min(1024, ceil(n_pad / 2048)) workgroups, each over its own
//       CONTIGUOUS run of indices, 16-byte loads; share b = the largest |g_i| of the run and its first index, and the run's NaN-ignoring max (the
//       convergence test's fold starts from -inf, the direction's from 0).  Stage two -- the shares folded in index order with the same strict > --
//       and the one-hot d are the control kernel's (QN_ST_AFTER_STEEP).
#pragma once

#define QN_PN_TPB 256
#define QN_PN_CH 4096     // columns of g staged in LDS per chunk
#define QN_PN_SHARE 8     // rows per share of g.d / ||g||_inf / non-finite count
#define QN_CD_SPAN 2048   // indices per workgroup of cd_argmax_kernel at most 1024 workgroups; beyond that the runs grow
#define QN_CD_NOIDX 0x7fffffff

struct QnPnormArgs {
    const double* P; // row-major, leading dimension n_pad
    const double* g; // n_pad
    double* d;       // n_pad
    double* part;    // [3][nshare]: g.d, ||g||_inf, number of non-finite d_i
    int n, n_pad, nshare;
};

template <bool NT>
__device__ __forceinline__ v2d qn_pn_ld(const double* p) {
    return NT ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p)) : ld2(p);
}

template <int RW, bool NT>
__global__ __launch_bounds__(QN_PN_TPB) void pnorm_dir_kernel(const QnPnormArgs a) {
    static_assert(RW == 2 || RW == 4, "rows per wave");
    constexpr int U = 8 / RW;          // column steps in flight
    constexpr int WROWS = 4 * RW;      // rows per workgroup
    __shared__ double gs[QN_PN_CH];
    __shared__ double dsh[WROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = a.n_pad, n = a.n;
    const int wg_row0 = blockIdx.x * WROWS;
    const int row0 = wg_row0 + wave * RW; // (< n_pad for every wave: n_pad is a multiple of 16, WROWS divides 16)
    const double* prow[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) prow[r] = a.P + (size_t)(row0 + r) * (size_t)np;
    double acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = 0.0;
    for (int c0 = 0; c0 < np; c0 += QN_PN_CH) {
        const int clen = min(QN_PN_CH, np - c0); // even: n_pad and QN_PN_CH are
        __syncthreads(); // (the waves have finished with the previous chunk)
        for (int j = 2 * tid; j < clen; j += 2 * QN_PN_TPB) {
            v2d gv = ld2(a.g + c0 + j);
            gv.x = (c0 + j < n) ? gv.x : 0.0;     // padding stays out of the sums
            gv.y = (c0 + j + 1 < n) ? gv.y : 0.0;
            *reinterpret_cast<v2d*>(gs + j) = gv;
        }
        __syncthreads();
        for (int j0 = 2 * lane; j0 < clen; j0 += 128 * U) {
            v2d h[U][RW], gv[U];
            bool in[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + 128 * u;
                in[u] = j < clen;
                const int jc = in[u] ? j : 0; // (past the chunk: a harmless re-read, masked below)
#pragma unroll
                for (int r = 0; r < RW; ++r) h[u][r] = qn_pn_ld<NT>(prow[r] + c0 + jc);
                gv[u] = *reinterpret_cast<const v2d*>(gs + jc);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = c0 + j0 + 128 * u;
                const bool k0 = in[u] && j < n, k1 = in[u] && j + 1 < n;
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const double hx = k0 ? h[u][r].x : 0.0, hy = k1 ? h[u][r].y : 0.0; // (a select, not a product with zero: the padding may hold anything)
                    const double gx = k0 ? gv[u].x : 0.0, gy = k1 ? gv[u].y : 0.0;
                    acc[r] = __builtin_fma(hx, gx, acc[r]); // FMA asked for: one rounding per term
                    acc[r] = __builtin_fma(hy, gy, acc[r]);
                }
            }
        }
    }
    // row sums: after the fold lane l holds the total of row (l >> SH) in acc[0]
    QnWaveFold<RW, 32>::run(acc, lane);
    constexpr int SH = 6 - qn_log2<RW>();
    if ((lane & ((1 << SH) - 1)) == 0) {
        const int r = lane >> SH, i = row0 + r;
        const double di = (i < n) ? -acc[0] : 0.0; // -(P g)_i, an exact negation
        a.d[i] = di;
        dsh[wave * RW + r] = di;
    }
    __syncthreads();
    if (tid < WROWS / QN_PN_SHARE) { // the shares: rows in ascending order
        const int r0 = tid * QN_PN_SHARE;
        double gd = 0.0, m = -INFINITY, nf = 0.0;
#pragma unroll
        for (int r = 0; r < QN_PN_SHARE; ++r) {
            const int i = wg_row0 + r0 + r;
            if (i < n) {
                const double gi = a.g[i], di = dsh[r0 + r];
                gd = __builtin_fma(gi, di, gd);  // FMA asked for
                m = fmax(fabs(gi), m);           // fold(NEG_INFINITY, |acc, x| x.abs().max(acc)): NaN entries are ignored (pnorm_descent.rs:56-58)
                nf += isfinite(di) ? 0.0 : 1.0;
            }
        }
        const int sh = (wg_row0 + r0) / QN_PN_SHARE;
        a.part[sh] = gd;
        a.part[(size_t)a.nshare + sh] = m;
        a.part[2 * (size_t)a.nshare + sh] = nf;
    }
}

// (magnitude, index) pairs: `b` replaces `a` when it is larger, or as large with a smaller index -- the order-free form of "the first index of
// the largest magnitude" (coordinate_descent.rs:35-41: replaced on `g.abs() > max` only).  A NaN magnitude compares false both ways and never wins.
__device__ __forceinline__ void qn_argmax_take(double& m, int& ix, const double m2, const int i2) {
    if (m2 > m || (m2 == m && i2 < ix)) { m = m2; ix = i2; }
}

struct QnCdArgs {
    const double* g;
    double* part; // [3][G]: largest magnitude, its first index (QN_CD_NOIDX: nothing in the run is > 0), NaN-ignoring max from -inf
    int n, span, G;
};

__global__ __launch_bounds__(256) void cd_argmax_kernel(const QnCdArgs a) {
    __shared__ double lm[4], lg[4];
    __shared__ int li[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * a.span, b1 = min(a.n, b0 + a.span); // (span is a multiple of 512, the vectors are n_pad long: a pair that starts below n is allocated)
    double m = 0.0, gm = -INFINITY; // the fold starts at (0, 0.0)
    int ix = QN_CD_NOIDX;
    for (int j = b0 + 2 * tid; j < b1; j += 512) {
        const v2d gv = ld2(a.g + j);
        const double a0 = fabs(gv.x), a1 = fabs(gv.y);
        if (a0 > m) { m = a0; ix = j; }
        gm = fmax(a0, gm);
        if (j + 1 < b1) {
            if (a1 > m) { m = a1; ix = j + 1; }
            gm = fmax(a1, gm);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double m2 = __shfl_xor(m, off, 64);
        const int i2 = __shfl_xor(ix, off, 64);
        qn_argmax_take(m, ix, m2, i2);
        gm = fmax(gm, __shfl_xor(gm, off, 64));
    }
    if (lane == 0) { lm[wave] = m; li[wave] = ix; lg[wave] = gm; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) { qn_argmax_take(m, ix, lm[w], li[w]); gm = fmax(gm, lg[w]); }
        a.part[blockIdx.x] = m;
        a.part[(size_t)a.G + blockIdx.x] = (double)ix;
        a.part[2 * (size_t)a.G + blockIdx.x] = gm;
    }
}
