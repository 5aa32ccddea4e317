// qn_multinomial.hip.h -- the regularised softmax-regression objective (OBJ_MULTINOMIAL) on a dense row-major A (m x n), labels y_i in {0, .., K-1},
// sample weights w_i >= 0, one rank.  The parameter vector is CLASS-MAJOR, x[k n + j] = W[k, j], N = K n entries without padding between classes
// (sklearn's coef_ raveled); g and H v have the same layout.  N_pad = make_tile(K n) <= 16384: W stays on chip.
//
//     z_ik = a_i . W_k,   p_i = softmax_k(z_i),   f = sum_i w_i (logsumexp_k z_ik - z_{i,y_i}) + mu/2 ||x||^2
//     g_k = sum_i w_i (p_ik - [y_i = k]) a_i + mu W_k,      (H v)_k = sum_i t_ik a_i + mu V_k,   t_ik = w_i p_ik (u_ik - sum_l p_il u_il),  u_ik = a_i . V_k
//
//   mnl_onepass_kernel<KC, NC>   ONE stream of A serves all K classes.  512 threads cut as TK x TJ (TJ = 64 .. 512 lanes over the columns, a wave never
//                                straddles two class groups): thread (tk, tj) owns the classes k = tk + TK i (i < KC) and the columns j = tj + TJ c
//                                (c < NC), and with them the KC x NC block of G in registers.  The workgroup's rows (lse_onepass_kernel's cut) go by in
//                                tiles of R = min(8, 16 / NC) rows (RT <= R of them in use: mnl_plan); a thread holds its R x NC entries of the tile and of the prefetched tile in registers
//                                (predicated loads past the row end and past the cut: zeros).  W (or V) sits in LDS at k n + j -- any parity of n.
//                                Per tile:
//                                  1. margins: per class, ONE LDS read of W_kj feeds R FMAs (chain over c in order); the R x KB partials of a class block
//                                     cross the wave in a halving butterfly (mnl_wave_reduce: lane pairs at distance 1, 2, 4, .. exchange one half and
//                                     add -- a fixed tree), the TJ / 64 waves of a class group are added in wave order.
//                                  2. wave r takes row r of the tile, lane l its classes l, l + 64, ..  The RULES PER ROW:
//                                       zmax = max_k z_k (this row's own K margins: no running maximum across rows)
//                                       e_k = exp(z_k - zmax);   S = sum_k e_k in CLASS ORDER (plain adds);   p_k = e_k / S (IEEE division)
//                                       l = (zmax - z_y) + log(S)
//                                       c_k = w p_k (k != y);   c_y = -(w (Sn / S)),  Sn = sum_{k != y} e_k in class order -- never w (p_y - 1), which
//                                             cancels where the row is fitted
//                                       w = 0: l = 0, c_k = 0 and the stored P_k = 0 BY SELECTS -- a masked row adds exactly nothing wherever it falls in
//                                             the cut, even where its margins overflowed from finite entries of A
//                                     Nothing overflows for finite margins (z_k - zmax <= 0, S in [1, K]); at a spread of 1600 the losers' e, p are 0.0.
//                                     Evaluation mode stores P (m x K) into the buffer given; F += w l in ROW ORDER (thread 0, plain adds).
//                                     PRODUCT mode (V in LDS, z = u): p_k read from the stored P, ubar = sum_k p_k u_k (FMA chain in class order),
//                                     c_k = (w p_k)(u_k - ubar); no transcendental function; F = 0.
//                                  3. G[k][j] += c_rk a_rj (FMA, rows in order; the coefficient is one broadcast LDS read for NC columns).
//                                Each workgroup writes (F, G) as [workgroup][N_pad] -- the layout logit_combine_kernel and lse_hv_combine_kernel (gbar =
//                                zeros) already fold: TWO launches per evaluation and per product, nothing new behind the stream.  A workgroup that owns
//                                no row writes zeros.
//   mnl_mfma_kernel<CTW>         the same stream on v_mfma_f64_16x16x4_f64 for K <= 64 (its own head comment below); which of the two an objective uses:
//                                qn_host_multinomial.hip.h (mnl_auto_kernel, qn_multinomial_set_kernel).
// No atomics, no workgroup waits for another, every order is fixed: the same bits for the same x from run to run and from object to object.
#pragma once

struct QnMnlArgs {
    const double* A;  // [mrpr][nfp]
    const double* wt; // m_pad sample weights, zero past m
    const int* lab;   // m_pad labels
    double* P;        // m x K: written in evaluation mode, read in product mode
    int m, mrpr, nf, nfp, K, N, N_pad;
    int tj_log2;      // TJ = 1 << tj_log2 (6 .. 9)
    int rt;           // rows of a tile in use (1 .. R): R unless the rows' scratch would not fit beside W (mnl_plan)
    int wk_log2;      // mnl_mfma_kernel: WK = 1 << wk_log2 class tiles of 16 classes (0 .. 2)
    int product;      // 0: evaluation at x, 1: product with v
};

// V values per lane (a power of two), summed over the 64 lanes of a wave in a fixed tree.  Halving steps at lane distance 1, 2, 4, ..: the lane whose bit
// is 0 keeps the lower half of what it holds and receives the partner's lower half, the other lane the upper halves.  Steps that are left once a lane
// holds a single value are plain butterflies (a + b in both lanes: the same bits).  Afterwards v[i], i < max(1, V / 64), holds the wave's total of the
// value with index i + sum_s bit_s(lane) (V >> (s + 1)) over the halving steps s.
template <int V, int CNT, int S>
__device__ __forceinline__ void mnl_wave_reduce_step(double (&v)[V], int lane) {
    if constexpr (S < 6) {
        if constexpr (CNT > 1) {
            constexpr int half = CNT / 2;
            const bool up = (lane >> S) & 1;
#pragma unroll
            for (int i = 0; i < half; ++i) {
                const double keep = up ? v[i + half] : v[i];
                const double send = up ? v[i] : v[i + half];
                v[i] = keep + __shfl_xor(send, 1 << S);
            }
            mnl_wave_reduce_step<V, half, S + 1>(v, lane);
        } else {
            v[0] = v[0] + __shfl_xor(v[0], 1 << S);
            mnl_wave_reduce_step<V, 1, S + 1>(v, lane);
        }
    }
}
template <int V>
__device__ __forceinline__ void mnl_wave_reduce(double (&v)[V], int lane) { mnl_wave_reduce_step<V, V, 0>(v, lane); }
template <int V>
__device__ __forceinline__ int mnl_reduce_index(int lane) {
    int idx = 0, cnt = V;
#pragma unroll
    for (int s = 0; s < 6; ++s)
        if (cnt > 1) { cnt /= 2; idx += ((lane >> s) & 1) * cnt; }
    return idx;
}
template <int V>
__device__ __forceinline__ bool mnl_reduce_writer(int lane) {
    int h = 0;
    for (int c = V; c > 1 && h < 6; c /= 2) ++h;
    return (lane >> h) == 0;
}

template <int KC, int NC>
__global__ __launch_bounds__(512) void mnl_onepass_kernel(const QnMnlArgs a, const double* __restrict__ x, double* __restrict__ wgf, double* __restrict__ wgg,
                                                          const QnVecCtl* __restrict__ ctl) {
    if (ctl && (ctl->phase != QN_VP_NSOLVE || ctl->method != QN_NEWTON_CG || ctl->tn_state != QN_TN_RUNNING)) return; // (lse_hv_onepass_kernel's rule)
    constexpr int R = 16 / NC < 8 ? 16 / NC : 8;        // rows per tile
    constexpr int VMAX = KC * NC >= 32 ? 16 : 32;       // partial sums in flight: fewer where G takes 64 registers or more
    constexpr int KB = KC < VMAX / R ? KC : VMAX / R;   // classes per block of the margins' reduction
    constexpr int V = R * KB;
    extern __shared__ __attribute__((aligned(16))) double mnl_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int TJ = 1 << a.tj_log2, TK = 512 >> a.tj_log2, WQ = TJ >> 6;
    const int tj = tid & (TJ - 1), tk = tid >> a.tj_log2;
    const int wq = wave & (WQ - 1); // this wave's place among the waves of its class group
    const int K = a.K, nf = a.nf, RT = a.rt;
    double* Wl = mnl_lds;                                  // N entries: W (or V), class-major
    double* zpart = mnl_lds + ((a.N + 1) & ~1);            // [WQ][RT][K]: the waves' shares of the margins; [0][r][k] then holds z_rk
    double* ebuf = zpart + (size_t)WQ * RT * K;            // [RT][K]: e_rk (product mode: p_rk)
    double* cbuf = ebuf + (size_t)RT * K;                  // [RT][K]: the coefficients c_rk
    double* lrow = cbuf + (size_t)RT * K;                  // [8]: the rows' loss terms
    for (int i = tid; i < a.N; i += 512) Wl[i] = x[i];
    __syncthreads();
    const int G = gridDim.x, per = (a.mrpr + G - 1) / G;
    const int r_lo = blockIdx.x * per;
    const int r_hi = min(min(a.mrpr, r_lo + per), a.m); // (rows past m are padding; one rank)
    // column slot c of this thread: tj + TJ c.  Past the row end NOTHING is loaded; the row's base is uniform (a scalar), tj the lane's offset
#define QN_MNL_IN(c) (tj + TJ * (c) < nf)
#define QN_MNL_LD(row, c) ((a.A + (size_t)(row) * a.nfp + TJ * (c))[tj])
    double g[KC][NC], cur[R][NC], nxt[R][NC];
#pragma unroll
    for (int i = 0; i < KC; ++i)
#pragma unroll
        for (int c = 0; c < NC; ++c) g[i][c] = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            cur[r][c] = 0.0;
            if (r < RT && r_lo + r < r_hi && QN_MNL_IN(c)) cur[r][c] = QN_MNL_LD(r_lo + r, c);
        }
    double f_run = 0.0;
    for (int r0 = r_lo; r0 < r_hi; r0 += RT) {
        // 1. the margins' shares of this wave
#pragma unroll 1
        for (int b = 0; b < KC / KB; ++b) {
            double v[V];
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = 0.0;
#pragma unroll
            for (int i = 0; i < KB; ++i) {
                const int k = tk + TK * (b * KB + i);
                const bool kin = k < K;
                const double* wk = Wl + (size_t)(kin ? k : 0) * nf;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const double wv = (kin && QN_MNL_IN(c)) ? wk[tj + TJ * c] : 0.0;
#pragma unroll
                    for (int r = 0; r < R; ++r) v[r * KB + i] = __builtin_fma(cur[r][c], wv, v[r * KB + i]);
                }
            }
            mnl_wave_reduce<V>(v, lane);
            if (mnl_reduce_writer<V>(lane)) {
                const int base = mnl_reduce_index<V>(lane);
#pragma unroll
                for (int i = 0; i < (V / 64 > 1 ? V / 64 : 1); ++i) {
                    const int idx = base + i, r = idx / KB, k = tk + TK * (b * KB + idx % KB);
                    if (k < K && r < RT) zpart[((size_t)wq * RT + r) * K + k] = v[i];
                }
            }
        }
        __syncthreads();
        // the next tile, on its way behind the margins (their partial sums are dead: the registers are these) while the rows' terms are formed
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                nxt[r][c] = 0.0;
                if (r < RT && r0 + RT + r < r_hi && QN_MNL_IN(c)) nxt[r][c] = QN_MNL_LD(r0 + RT + r, c);
            }
        // 2. wave r: row r of the tile
        const int row = r0 + wave;
        const bool mine = wave < RT;
        const bool valid = mine && row < r_hi;
        const double wg = valid ? a.wt[row] : 0.0;
        const int y = valid ? a.lab[row] : 0;
        double* zr = zpart + (size_t)(mine ? wave : 0) * K;
        double* er = ebuf + (size_t)(mine ? wave : 0) * K;
        double* cr = cbuf + (size_t)(mine ? wave : 0) * K;
        double zmax = -INFINITY;
        if (mine) {
            for (int k = lane; k < K; k += 64) {
                double z = zr[k];
                for (int q = 1; q < WQ; ++q) z = z + zr[(size_t)q * RT * K + k];
                zr[k] = z;
                zmax = fmax(zmax, z);
            }
#pragma unroll
            for (int s = 1; s < 64; s *= 2) zmax = fmax(zmax, __shfl_xor(zmax, s));
            for (int k = lane; k < K; k += 64) {
                if (a.product) er[k] = valid ? a.P[(size_t)row * K + k] : 0.0;
                else er[k] = exp(zr[k] - zmax);
            }
        }
        __syncthreads();
        if (mine) {
            if (!a.product) {
                double S = 0.0, Sn = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double e = er[k];
                    S = S + e;
                    Sn = Sn + (k == y ? 0.0 : e);
                }
                const double cy = -(wg * (Sn / S));
                for (int k = lane; k < K; k += 64) {
                    const double p = er[k] / S;
                    const double ck = k == y ? cy : wg * p;
                    cr[k] = wg == 0.0 ? 0.0 : ck;
                    if (valid) a.P[(size_t)row * K + k] = wg == 0.0 ? 0.0 : p;
                }
                if (lane == 0) {
                    const double l = (zmax - zr[y]) + log(S);
                    lrow[wave] = wg == 0.0 ? 0.0 : wg * l;
                }
            } else {
                double ub = 0.0;
                for (int k = 0; k < K; ++k) ub = __builtin_fma(er[k], zr[k], ub);
                for (int k = lane; k < K; k += 64) {
                    const double t = (wg * er[k]) * (zr[k] - ub);
                    cr[k] = wg == 0.0 ? 0.0 : t;
                }
                if (lane == 0) lrow[wave] = 0.0;
            }
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < RT; ++r) f_run = f_run + lrow[r];
        // 3. G += c_rk a_rj
#pragma unroll
        for (int i = 0; i < KC; ++i) {
            const int k = tk + TK * i;
            if (k < K) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double ck = r < RT ? cbuf[(size_t)r * K + k] : 0.0; // (rows past RT are zeros in `cur`)
#pragma unroll
                    for (int c = 0; c < NC; ++c) g[i][c] = __builtin_fma(ck, cur[r][c], g[i][c]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) cur[r][c] = nxt[r][c];
    }
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        const int k = tk + TK * i;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (k < K && QN_MNL_IN(c)) wgg[(size_t)blockIdx.x * a.N_pad + (size_t)k * nf + tj + TJ * c] = g[i][c];
    }
    if (tid == 0) wgf[blockIdx.x] = f_run;
#undef QN_MNL_IN
#undef QN_MNL_LD
}

// mnl_mfma_kernel<CTW>: the same objective, rules per row, share layout and guarantees on v_mfma_f64_16x16x4_f64, for K <= 64 (qn_lse_hess.hip.h has the
// operand layout: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[i = (lane >> 4) + 4 reg][j = lane & 15]).  Tiles of 16 rows.  The
// eight waves are cut as WK class tiles of 16 classes (WK = 1, 2, 4) x WC = 8 / WK column groups; wave (wk, wc) owns the class tile wk and the column
// tiles ct = wc + WC i (i < CTW) of 16 columns, and with them CTW 16 x 16 blocks of G in 4 CTW accumulators a lane.  W (or V) sits in LDS with a class
// pitch of n_pad + 2 doubles (zeros past n): the 16 classes of a quarter wave then start 4 banks apart and a 32-byte read is conflict-free.  Per tile:
//   1. margins Z'[k][r] = sum_j W[k][j] A[r][j]: per column tile four MFMAs; lane (l4, l15) holds the four consecutive entries j = c0 + 4 l4 + s of
//      class l15 (from LDS) and of row l15 (from memory, 128 contiguous bytes a row) -- MFMA s contracts the columns c0 + 4 l4 + s, l4 = 0 .. 3, the
//      same map on both operands.  The column groups' shares are added in group order through LDS.
//   2. wave w takes the rows w and w + 8 of the tile, lane l the class l: mnl_onepass_kernel's rules, sum for sum.
//   3. G[k][j] += sum_r c[r][k] A[r][j]: four MFMAs per column tile, the rows 4 s + l4 contracted; A comes from memory a second time in this layout
//      (16 consecutive doubles of a row a quarter wave: the tile was read by this workgroup a moment ago -- one stream of A from HBM).
// Three barriers per 16 rows.  Every sum in a fixed order (the MFMA's own, the groups', the classes'); no atomics; predicated loads past the cut.
template <int CTW>
__global__ __launch_bounds__(512) void mnl_mfma_kernel(const QnMnlArgs a, const double* __restrict__ x, double* __restrict__ wgf, double* __restrict__ wgg,
                                                       const QnVecCtl* __restrict__ ctl) {
    if (ctl && (ctl->phase != QN_VP_NSOLVE || ctl->method != QN_NEWTON_CG || ctl->tn_state != QN_TN_RUNNING)) return;
    extern __shared__ __attribute__((aligned(16))) double mnl_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int WK = 1 << a.wk_log2, WC = 8 >> a.wk_log2, KP = 16 * WK;
    const int wk = wave & (WK - 1), wc = wave >> a.wk_log2;
    const int K = a.K, nf = a.nf, nfp = a.nfp, pitch = a.nfp + 2;
    double* Wl = mnl_lds;                            // [K][pitch]
    double* zpart = Wl + (size_t)K * pitch;          // [WC][KP][16]: the column groups' shares of Z'; [0][k][r] then holds z_rk
    double* ebuf = zpart + (size_t)KP * 16;          // = zpart[1]: e_rk (product mode: p_rk) takes the place of the share it was added from
    double* cbuf = zpart + (size_t)WC * KP * 16;     // [16][KP]: the coefficients c_rk
    double* lrow = cbuf + (size_t)16 * KP;           // [16]: the rows' loss terms
    for (int i = tid; i < K * pitch; i += 512) {
        const int k = i / pitch, j = i - k * pitch;
        Wl[i] = j < nf ? x[(size_t)k * nf + j] : 0.0;
    }
    __syncthreads();
    const int G = gridDim.x, per = (a.mrpr + G - 1) / G;
    const int r_lo = blockIdx.x * per;
    const int r_hi = min(min(a.mrpr, r_lo + per), a.m);
    const int kmine = 16 * wk + l15; // the class this lane feeds to both products
    v4d acc[CTW];
#pragma unroll
    for (int i = 0; i < CTW; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double f_run = 0.0;
    for (int r0 = r_lo; r0 < r_hi; r0 += 16) {
        // 1. this wave's share of Z'
        v4d z = {0.0, 0.0, 0.0, 0.0};
        {
            const bool rin = r0 + l15 < r_hi;
            const double* arow = a.A + (size_t)(rin ? r0 + l15 : 0) * nfp + 4 * l4;
            const double* wrow = Wl + (size_t)(kmine < K ? kmine : 0) * pitch + 4 * l4;
#pragma unroll
            for (int i = 0; i < CTW; ++i) {
                const int c0 = 16 * (wc + WC * i);
                if (c0 < nfp) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double av = rin ? arow[c0 + q] : 0.0;
                        const double wv = kmine < K ? wrow[c0 + q] : 0.0;
                        z = __builtin_amdgcn_mfma_f64_16x16x4f64(wv, av, z, 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) zpart[((size_t)wc * KP + 16 * wk + l4 + 4 * q) * 16 + l15] = z[q];
        __syncthreads();
        // 2. the rows `wave` and `wave + 8` of the tile; lane = class
        const bool kin = lane < K, kst = lane < KP;
        double zk[2], zm[2], eo[2], wgt[2];
        int yy[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int rr = wave + 8 * h, row = r0 + rr;
            const bool valid = row < r_hi;
            wgt[h] = valid ? a.wt[row] : 0.0;
            yy[h] = valid ? a.lab[row] : 0;
            double zz = 0.0;
            if (kst) {
                zz = zpart[(size_t)lane * 16 + rr];
                for (int q = 1; q < WC; ++q) zz = zz + zpart[((size_t)q * KP + lane) * 16 + rr];
                zpart[(size_t)lane * 16 + rr] = zz;
            }
            double zmax = kin ? zz : -INFINITY;
#pragma unroll
            for (int sft = 1; sft < 64; sft *= 2) zmax = fmax(zmax, __shfl_xor(zmax, sft));
            double e = 0.0;
            if (kin) e = a.product ? (valid ? a.P[(size_t)row * K + lane] : 0.0) : exp(zz - zmax);
            if (kst) ebuf[(size_t)lane * 16 + rr] = e;
            zk[h] = zz; zm[h] = zmax; eo[h] = e;
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int rr = wave + 8 * h, row = r0 + rr;
            const bool valid = row < r_hi;
            const double wg = wgt[h];
            const int y = yy[h];
            double ck = 0.0;
            if (!a.product) {
                double S = 0.0, Sn = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double e = ebuf[(size_t)k * 16 + rr];
                    S = S + e;
                    Sn = Sn + (k == y ? 0.0 : e);
                }
                const double cy = -(wg * (Sn / S));
                const double p = eo[h] / S;
                ck = lane == y ? cy : wg * p;
                if (valid && kin) a.P[(size_t)row * K + lane] = wg == 0.0 ? 0.0 : p;
                const double zy = __shfl(zk[h], y);
                if (lane == 0) {
                    const double l = (zm[h] - zy) + log(S);
                    lrow[rr] = wg == 0.0 ? 0.0 : wg * l;
                }
            } else {
                double ub = 0.0;
                for (int k = 0; k < K; ++k) ub = __builtin_fma(ebuf[(size_t)k * 16 + rr], zpart[(size_t)k * 16 + rr], ub);
                ck = (wg * eo[h]) * (zk[h] - ub);
                if (lane == 0) lrow[rr] = 0.0;
            }
            if (kst) cbuf[(size_t)rr * KP + lane] = (wg == 0.0 || !kin) ? 0.0 : ck;
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < 16; ++r) f_run = f_run + lrow[r];
        // 3. G += c' A
        {
            double cv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) cv[q] = cbuf[(size_t)(4 * q + l4) * KP + 16 * wk + l15];
#pragma unroll
            for (int i = 0; i < CTW; ++i) {
                const int c0 = 16 * (wc + WC * i);
                if (c0 < nfp) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = r0 + 4 * q + l4;
                        const double bv = row < r_hi ? a.A[(size_t)row * nfp + c0 + l15] : 0.0;
                        acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv[q], bv, acc[i], 0, 0, 0);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < CTW; ++i) {
        const int col = 16 * (wc + WC * i) + l15;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 16 * wk + l4 + 4 * q;
            if (k < K && col < nf) wgg[(size_t)blockIdx.x * a.N_pad + (size_t)k * nf + col] = acc[i][q];
        }
    }
    if (tid == 0) wgf[blockIdx.x] = f_run;
}

// the cut of the 512 threads and the instance for (n, K): TJ lanes over the columns, NC = columns per thread, KC = classes per thread, both rounded up
// to a power of two.  Among the cuts that fit (KC <= 32, NC <= 16, KC NC <= 64) the one with at most 32 accumulators, at most four class groups (each
// group loads the tile again) and NC closest to 4 (R = 4 rows per LDS read of W, four FMAs per coefficient) is taken; ties go to the wider TJ.
// The rows' scratch, (WQ + 2) RT K + 8 doubles, lies beside W in the workgroup's 160 KiB of LDS: RT is R, halved until it fits (K >= 128 with N_pad close
// to 16384: 2 rows at worst; every (n, K) with K n <= 16384 and K <= 256 fits at RT = 1, so no shape inside the limits is left without a cut).  The rows
// past RT of a tile stay zeros in registers: such a shape pays the FMAs of R rows for RT.
constexpr size_t QN_MNL_LDS_MAX = 160 * 1024; // what one workgroup can get on gfx950
static size_t mnl_lds_bytes(const QnMnlPlan& p, int N, int K) {
    return ((size_t)((N + 1) & ~1) + (size_t)(p.WQ + 2) * p.RT * K + 8) * sizeof(double);
}
static int mnl_pow2ceil(int v) { int p = 1; while (p < v) p *= 2; return p; }
static QnMnlPlan mnl_plan(int nf, int K) {
    QnMnlPlan best{0, 0, 0, 0, 0, 0, false};
    long best_score = -1;
    for (int t = 9; t >= 6; --t) {
        const int TJ = 1 << t, TK = 512 >> t;
        const int NC = mnl_pow2ceil((nf + TJ - 1) / TJ), KC = std::max(2, mnl_pow2ceil((K + TK - 1) / TK));
        if (NC > 16 || KC > 32 || KC * NC > 64) continue;
        int dist = 0;
        for (int v = NC; v < 4; v *= 2) ++dist;
        for (int v = NC; v > 4; v /= 2) ++dist;
        long score = (KC * NC <= 32 ? 1000 : 0) + (TK <= 4 ? 100 : 0) + 10 * (4 - dist);
        if (score > best_score) {
            best_score = score;
            const int R = 16 / NC < 8 ? 16 / NC : 8;
            best = QnMnlPlan{t, KC, NC, R, R, TJ >> 6, true};
        }
    }
    if (!best.ok) return best;
    while (best.RT > 1 && mnl_lds_bytes(best, nf * K, K) > QN_MNL_LDS_MAX) best.RT /= 2;
    best.ok = mnl_lds_bytes(best, nf * K, K) <= QN_MNL_LDS_MAX;
    return best;
}

template <int KC, int NC>
static int mnl_launch_inst(hipStream_t st, int G, size_t lds, const QnMnlArgs& a, const double* x, double* wgf, double* wgg, const QnVecCtl* ctl) {
    static std::atomic<size_t> attr_set[64]; // per device, as lse_launch_onepass_nt: the largest LDS size granted so far
    int dev = 0;
    (void)hipGetDevice(&dev);
    if ((dev < 0 || dev >= 64 || attr_set[dev].load() < lds) && lds > 48 * 1024) {
        if (hipFuncSetAttribute((const void*)mnl_onepass_kernel<KC, NC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return fail(QN_ERROR_INPUT_PARAMS, "the multinomial objective is not built for this device: it does not grant the LDS that holds W");
        }
        if (dev >= 0 && dev < 64) attr_set[dev].store(lds);
    }
    hipLaunchKernelGGL((mnl_onepass_kernel<KC, NC>), dim3(G), dim3(512), lds, st, a, x, wgf, wgg, ctl);
    return QN_OK;
}
template <int NC>
static int mnl_launch_nc(hipStream_t st, int G, size_t lds, int KC, const QnMnlArgs& a, const double* x, double* wgf, double* wgg, const QnVecCtl* ctl) {
    switch (KC) {
    case 2: return mnl_launch_inst<2, NC>(st, G, lds, a, x, wgf, wgg, ctl);
    case 4: return mnl_launch_inst<4, NC>(st, G, lds, a, x, wgf, wgg, ctl);
    case 8: if constexpr (NC <= 8) return mnl_launch_inst<8, NC>(st, G, lds, a, x, wgf, wgg, ctl); break;
    case 16: if constexpr (NC <= 4) return mnl_launch_inst<16, NC>(st, G, lds, a, x, wgf, wgg, ctl); break;
    case 32: if constexpr (NC <= 2) return mnl_launch_inst<32, NC>(st, G, lds, a, x, wgf, wgg, ctl); break;
    }
    return fail(QN_ERROR_INPUT_PARAMS, "the multinomial objective has no kernel instance for this cut");
}
static int mnl_launch(hipStream_t st, int G, const QnMnlPlan& p, const QnMnlArgs& a, const double* x, double* wgf, double* wgg, const QnVecCtl* ctl) {
    const size_t lds = mnl_lds_bytes(p, a.N, a.K);
    switch (p.NC) {
    case 1: return mnl_launch_nc<1>(st, G, lds, p.KC, a, x, wgf, wgg, ctl);
    case 2: return mnl_launch_nc<2>(st, G, lds, p.KC, a, x, wgf, wgg, ctl);
    case 4: return mnl_launch_nc<4>(st, G, lds, p.KC, a, x, wgf, wgg, ctl);
    case 8: return mnl_launch_nc<8>(st, G, lds, p.KC, a, x, wgf, wgg, ctl);
    default: return mnl_launch_nc<16>(st, G, lds, p.KC, a, x, wgf, wgg, ctl);
    }
}

// mnl_mfma_kernel's cut for (n_pad, K), K <= 64: WK class tiles x WC column groups, CTW column tiles a wave (a power of two, at most 16)
static QnMnlMfmaPlan mnl_mfma_plan(int nfp, int K) {
    QnMnlMfmaPlan p{0, 0, 0, false};
    if (K > 64) return p;
    const int KT = (K + 15) / 16, WK = mnl_pow2ceil(KT), WC = 8 / WK, NT = nfp / 16;
    p.wk_log2 = WK == 1 ? 0 : WK == 2 ? 1 : 2;
    p.CTW = mnl_pow2ceil((NT + WC - 1) / WC);
    p.lds = ((size_t)K * (nfp + 2) + (size_t)WC * 16 * WK * 16 + (size_t)16 * 16 * WK + 16) * sizeof(double);
    p.ok = p.CTW <= 16 && p.lds <= QN_MNL_LDS_MAX;
    return p;
}
template <int CTW>
static int mnl_mfma_launch_inst(hipStream_t st, int G, size_t lds, const QnMnlArgs& a, const double* x, double* wgf, double* wgg, const QnVecCtl* ctl) {
    static std::atomic<size_t> attr_set[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if ((dev < 0 || dev >= 64 || attr_set[dev].load() < lds) && lds > 48 * 1024) {
        if (hipFuncSetAttribute((const void*)mnl_mfma_kernel<CTW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return fail(QN_ERROR_INPUT_PARAMS, "the multinomial objective is not built for this device: it does not grant the LDS that holds W");
        }
        if (dev >= 0 && dev < 64) attr_set[dev].store(lds);
    }
    hipLaunchKernelGGL((mnl_mfma_kernel<CTW>), dim3(G), dim3(512), lds, st, a, x, wgf, wgg, ctl);
    return QN_OK;
}
static int mnl_mfma_launch(hipStream_t st, int G, const QnMnlMfmaPlan& p, const QnMnlArgs& a, const double* x, double* wgf, double* wgg, const QnVecCtl* ctl) {
    switch (p.CTW) {
    case 1: return mnl_mfma_launch_inst<1>(st, G, p.lds, a, x, wgf, wgg, ctl);
    case 2: return mnl_mfma_launch_inst<2>(st, G, p.lds, a, x, wgf, wgg, ctl);
    case 4: return mnl_mfma_launch_inst<4>(st, G, p.lds, a, x, wgf, wgg, ctl);
    case 8: return mnl_mfma_launch_inst<8>(st, G, p.lds, a, x, wgf, wgg, ctl);
    default: return mnl_mfma_launch_inst<16>(st, G, p.lds, a, x, wgf, wgg, ctl);
    }
}
