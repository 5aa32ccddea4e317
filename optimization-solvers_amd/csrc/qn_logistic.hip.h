// qn_logistic.hip.h -- the regularised logistic-regression objective (OBJ_LOGISTIC) on a dense row-major A (m x n, n_pad <= 16384, one rank):
//
//     f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2,      g = -A'(y o w o s) + mu x,      H = A' diag(d) A + mu I
//     z_i = y_i a_i'x,   s_i = 1 / (1 + exp(z_i)),   d_i = w_i s_i (1 - s_i),   y_i in {-1, +1},   w_i >= 0
//
// The device keeps yw_i = y_i w_i (the objective's `b`, m_pad entries, zero past m): the sign is the label, the magnitude the weight, and a row with
// yw_i = 0 is masked -- it adds nothing to f, g or H wherever it falls in the cut of the rows over workgroups (log-sum-exp's c_i = -inf).
//
//   logit_onepass_kernel<KCH, NTA>    lse_hv_onepass_kernel's sibling (qn_lse_hv.hip.h): its geometry (512 threads, the same row cut over os.G
//                                     workgroups), x staged in LDS, each thread's KCH x 2 columns of the current row, of the prefetched row and of G
//                                     in registers, predicated loads past n_pad, ONE barrier per row for u_r = a_r . x in lse_onepass_kernel's order
//                                     (FMA chain per thread, wave butterfly, eight partials added in index order), the same non-temporal rule for A.
//                                     A row's weight depends on its own margin only: no running maximum, no rescale of G, no global normalisation.
//                                     Per row, in this order:
//                                         z = sign(yw) u;  t = |z|;  e = exp(-t);  q = 1 + e;  s = z >= 0 ? e / q : 1 / q        (every thread)
//                                         coefficient = -(yw s);  G += coefficient a_r (FMA)                                      (every thread)
//                                         d = |yw| ((e / q) / q), stored into the m_pad buffer given; z stored beside it        (thread 64 alone)
//                                     and behind the stream, from the stored margins (e = exp(-|z|) again: the same bits):
//                                         l = |yw| (max(-z, 0) + log1p(e))               (one lane per row, 512 rows at a time)
//                                         F += l (plain adds, ROW ORDER)                 (thread 0 alone)
//                                     The divisions are IEEE divisions; yw = 0 gives l = coefficient = d = 0 by a select.  Nothing overflows for a
//                                     finite margin: t >= 0, e in [0, 1], q in [1, 2].  The all-threads path holds one exp and one division; the
//                                     second and third division run in one lane of one wave; log1p never meets the row loop's registers.
//                                     Each workgroup writes (F, G); one that owns no row writes zeros.
//   logit_combine_kernel              g_j = (sum_wg G_wg,j in lse_hv_combine_kernel's order: each quarter of the workgroups in workgroup order,
//                                     sixteen loads in flight, the quarters added in order, plain adds) + mu x_j, zero past n; workgroup 0 also
//                                     f = sum_wg F_wg (thread w holds share w, ctl_block_sum) + 0.5 mu ||x||^2 (sixteen loads in flight, FMA chain per
//                                     thread, ctl_block_sum -- lse_finish1_kernel's block 0).
// TWO launches per evaluation.  The Hessian-vector product needs no kernel of its own: with pw = d and a zero vector where gbar goes,
// lse_hv_onepass_kernel + lse_hv_combine_kernel compute A'(d o (A v)) + mu v exactly (S * 0 = 0, gs - 0 = gs bit for bit).
//
// No atomics, no workgroup waits for another, every order is fixed: the same bits for the same x from run to run and from object to object.
#pragma once

template <int KCH, bool NTA>
__global__ __launch_bounds__(512) void logit_onepass_kernel(const QnLseArgs a, const double* __restrict__ x, const double* __restrict__ yw,
                                                            double* __restrict__ d_out, double* __restrict__ z_out, double* __restrict__ wgf,
                                                            double* __restrict__ wgg) {
    extern __shared__ __attribute__((aligned(16))) double logit_x[]; // KCH * 1024 entries of x, zero past n
    __shared__ double red[2][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = a.n_pad;
    // column pair k of this thread: 2 tid + 1024 k.  Past the end NOTHING is loaded (lse_hv_onepass_kernel's predicate: a mask in scalar registers)
#define QN_LGT_IN(k) (2 * tid + 1024 * (k) < np)
#define QN_LGT_LD(row, k) (NTA ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>((row) + 1024 * (k) + 2 * tid)) : ld2((row) + 1024 * (k) + 2 * tid))
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int j = 2 * tid + 1024 * k;
        v2d xv = {0.0, 0.0};
        if (j < np) xv = ld2(x + j);
        logit_x[j] = j < a.n ? xv.x : 0.0; logit_x[j + 1] = j + 1 < a.n ? xv.y : 0.0;
    }
    __syncthreads();
    const int G = gridDim.x, per = (a.mrpr + G - 1) / G;
    const int r_lo = blockIdx.x * per;
    const int r_hi = min(min(a.mrpr, r_lo + per), a.m); // (rows past m are padding; one rank)
    v2d g[KCH], cur[KCH], nxt[KCH];
#pragma unroll
    for (int k = 0; k < KCH; ++k) { g[k] = (v2d){0.0, 0.0}; cur[k] = (v2d){0.0, 0.0}; }
    if (r_lo < r_hi) {
#pragma unroll
        for (int k = 0; k < KCH; ++k)
            if (QN_LGT_IN(k)) cur[k] = QN_LGT_LD(a.A + (size_t)r_lo * np, k);
    }
    for (int r = r_lo; r < r_hi; ++r) {
        const double* nrow = a.A + (size_t)((r + 1 < r_hi) ? r + 1 : r) * np; // (last row: a harmless re-read, no branch)
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            nxt[k] = (v2d){0.0, 0.0};
            if (QN_LGT_IN(k)) nxt[k] = QN_LGT_LD(nrow, k);
        }
        const double ywr = yw[r];
        double p = 0.0;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const int j = 2 * tid + 1024 * k;
            const v2d xv = *reinterpret_cast<const v2d*>(&logit_x[j]);
            p = __builtin_fma(cur[k].x, xv.x, p);
            p = __builtin_fma(cur[k].y, xv.y, p);
        }
        p = qn_wave_sum(p);
        if (lane == 0) red[r & 1][wave] = p;
        __syncthreads();
        double u = red[r & 1][0];
#pragma unroll
        for (int w = 1; w < 8; ++w) u = u + red[r & 1][w];
        const double z = ywr < 0.0 ? -u : u;
        const double t = fabs(z);
        const double e = exp(-t);
        const double q = 1.0 + e;
        const double s = (z >= 0.0 ? e : 1.0) / q; // (e / q or 1 / q: one division, the numerator selected)
        const double ys = ywr * s;
        const double coef = ywr == 0.0 ? 0.0 : -ys; // (a select, not a branch: a masked row adds nothing even where its u overflowed from finite entries of A)
        if (tid == 64) { // the Hessian's weight of this row, and its margin for the loss (below, behind the stream)
            const double dr = fabs(ywr) * ((e / q) / q);
            d_out[r] = ywr == 0.0 ? 0.0 : dr;
            z_out[r] = z;
        }
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            g[k].x = __builtin_fma(coef, cur[k].x, g[k].x);
            g[k].y = __builtin_fma(coef, cur[k].y, g[k].y);
            cur[k] = nxt[k];
        }
    }
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int j = 2 * tid + 1024 * k;
        if (j < np) st2(wgg + (size_t)blockIdx.x * np + j, g[k]);
    }
    // The loss, behind the stream: log1p inside the row loop costs the KCH = 16 instance 27 spilled registers (the row, the prefetched row and G are
    // 192 of its 256).  Here those are dead: 512 rows at a time, thread i takes row base + i -- e = exp(-|z|) again, the same bits --, and thread 0
    // adds the 512 terms in ROW ORDER with plain adds: the sum the row loop would have made.  (x in LDS is no longer needed: its first 512 entries
    // hold the terms.)
    double f_run = 0.0;
    for (int base = r_lo; base < r_hi; base += 512) {
        __syncthreads(); // the margins of this workgroup's rows are visible; the terms of the chunk before have been added
        const int r = base + tid;
        double l = 0.0;
        if (r < r_hi) {
            const double ywr = yw[r], z = z_out[r];
            const double e = exp(-fabs(z));
            const double lr = fabs(ywr) * (fmax(-z, 0.0) + log1p(e));
            l = ywr == 0.0 ? 0.0 : lr;
        }
        logit_x[tid] = l;
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(512, r_hi - base);
            for (int i = 0; i < cnt; ++i) f_run = f_run + logit_x[i];
        }
    }
    if (tid == 0) wgf[blockIdx.x] = f_run;
#undef QN_LGT_IN
#undef QN_LGT_LD
}

// 64 columns per workgroup, G <= 256 workgroups' results: see the head of this file
__global__ __launch_bounds__(256) void logit_combine_kernel(const QnLseArgs a, int G, const double* __restrict__ wgf, const double* __restrict__ wgg,
                                                            const double* __restrict__ x, double* __restrict__ f_out, double* __restrict__ g_out) {
    __shared__ double lds[32];
    __shared__ double part[3][64];
    const int tid = threadIdx.x;
    const int c = tid & 63, q = tid >> 6;
    const int col = blockIdx.x * 64 + c;
    const int j = min(col, a.n_pad - 1);
    const int per = (G + 3) / 4, w_lo = q * per, w_hi = min(G, w_lo + per);
    double acc = 0.0;
    for (int w0 = w_lo; w0 < w_hi; w0 += 16) {
        double t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = (w0 + u < w_hi) ? wgg[(size_t)(w0 + u) * a.n_pad + j] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = acc + t[u];
    }
    if (q > 0) part[q - 1][c] = acc;
    __syncthreads();
    if (q == 0) {
        if (col < a.n) {
            const double gs = ((acc + part[0][c]) + part[1][c]) + part[2][c];
            const double mx = a.mu * x[j];
            g_out[j] = gs + mx;
        } else if (col < a.n_pad) {
            g_out[j] = 0.0;
        }
    }
    if (blockIdx.x != 0) return;
    double p[2] = {tid < G ? wgf[tid] : 0.0, 0.0}; // thread w holds workgroup w's share of f; ||x||^2 beside it
    for (int j0 = tid; j0 < a.n; j0 += 16 * 256) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int jj = j0 + u * 256; v[u] = jj < a.n ? x[jj] : 0.0; }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (j0 + u * 256 < a.n) p[1] = __builtin_fma(v[u], v[u], p[1]);
    }
    ctl_block_sum<2>(p, lds);
    if (tid == 0) *f_out = p[0] + 0.5 * a.mu * p[1];
}

template <int KCH, bool NTA>
static int logit_launch_nt(hipStream_t st, int G, const QnLseArgs& a, const double* x, const double* yw, double* d_out, double* z_out, double* wgf, double* wgg) {
    static std::atomic<bool> attr_set[64]; // per device, as lse_launch_onepass_nt
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t lds = (size_t)KCH * 1024 * sizeof(double);
    if ((dev < 0 || dev >= 64 || !attr_set[dev].load()) && lds > 48 * 1024) {
        if (hipFuncSetAttribute((const void*)logit_onepass_kernel<KCH, NTA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return fail(QN_ERROR_INPUT_PARAMS, "the logistic objective is not built for this device: it does not grant the LDS that holds x");
        }
        if (dev >= 0 && dev < 64) attr_set[dev].store(true);
    }
    hipLaunchKernelGGL((logit_onepass_kernel<KCH, NTA>), dim3(G), dim3(512), lds, st, a, x, yw, d_out, z_out, wgf, wgg);
    return QN_OK;
}
template <int KCH>
static int logit_launch(hipStream_t st, int G, const QnLseArgs& a, const double* x, const double* yw, double* d_out, double* z_out, double* wgf, double* wgg) {
    // the log-sum-exp evaluation's rule: rows of A that cannot stay in the Infinity Cache between passes are requested as non-temporal (QN_LSE_NT = 0 / 1 overrides)
    static const int nt_env = getenv("QN_LSE_NT") ? atoi(getenv("QN_LSE_NT")) : -1;
    const bool nt = nt_env >= 0 ? nt_env != 0 : (size_t)a.mrpr * (size_t)a.n_pad * sizeof(double) > ((size_t)230 << 20);
    return nt ? logit_launch_nt<KCH, true>(st, G, a, x, yw, d_out, z_out, wgf, wgg) : logit_launch_nt<KCH, false>(st, G, a, x, yw, d_out, z_out, wgf, wgg);
}
