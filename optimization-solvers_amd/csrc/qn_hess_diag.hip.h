// qn_hess_diag.hip.h -- the diagonal of the Hessian of the dense kinds that stream A once per product (LogSumExp, Logistic), without the matrix:
//
//     M_j = H(x)_jj = sum_r pw_r a_rj^2 - gbar_j^2 + mu,      pw = p (log-sum-exp) or d (logistic),  gbar = A'p or zeros
//
// ONE stream of A (8 m n bytes, what one product moves), with the weights the kind's last weights pass left in `wp.w`.  It is what a Jacobi
// preconditioner of NewtonCG's inner loop divides by (qn_newton_cg.hip.h, rule 2'), and a public quantity (qn_objective_hess_diag_at).
//
//   hd_onepass_kernel<KCH, NTA>   lse_hv_onepass_kernel's sibling (qn_lse_hv.hip.h): its grid (512 threads, the same row cut over os.G workgroups),
//                                 its column ownership (pair k of thread tid: 2 tid + 1024 k), its predicated loads, its prefetched next row and
//                                 its non-temporal rule for A.  Nothing is staged in LDS and there is NO barrier per row: a row's term depends on its
//                                 own weight alone.  THE ROUNDING ORDER, per entry: s = a_rj a_rj (rounded), G_j = fma(pw_r, s, G_j), the rows of a
//                                 workgroup in index order.  A row with pw_r = 0 (masked, padding) adds nothing: G_j keeps its value by a select,
//                                 whatever a_rj is.  Each workgroup writes its G into os.wgg ([workgroup][n_pad], the product's shares: one stream,
//                                 and every pass rewrites all of it); one that owns no row writes zeros.
//   hd_combine_kernel             M_j = (sum_wg G_wg,j in lse_hv_combine_kernel's order: each quarter of the workgroups in workgroup order, sixteen
//                                 loads in flight, the quarters added in order) - gbar_j gbar_j (the product rounded on its own), + mu.  Where it is
//                                 given `minv` the same launch writes 1 / M_j by IEEE division when M_j > 0 and finite, else 1 (rule 2').  Entries
//                                 n .. n_pad: M = 0, minv = 1.
//
// No atomics, no workgroup waits for another, every order is fixed: the same bits for the same x from run to run and from object to object.
// Built where the product is (lse_hv_built: n_pad <= 16384, one rank).  Neither kernel is predicated: they write the objective's scratch and the
// caller's two vectors only.
#pragma once

template <int KCH, bool NTA>
__global__ __launch_bounds__(512) void hd_onepass_kernel(const QnLseArgs a, const double* __restrict__ pw, double* __restrict__ wgg) {
    const int tid = threadIdx.x;
    const int np = a.n_pad;
#define QN_HD_IN(k) (2 * tid + 1024 * (k) < np)
#define QN_HD_LD(row, k) (NTA ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>((row) + 1024 * (k) + 2 * tid)) : ld2((row) + 1024 * (k) + 2 * tid))
    const int G = gridDim.x, per = (a.mrpr + G - 1) / G;
    const int r_lo = blockIdx.x * per;
    const int r_hi = min(min(a.mrpr, r_lo + per), a.m - a.rank * a.mrpr); // (rows past m are padding)
    v2d g[KCH], cur[KCH], nxt[KCH];
#pragma unroll
    for (int k = 0; k < KCH; ++k) { g[k] = (v2d){0.0, 0.0}; cur[k] = (v2d){0.0, 0.0}; }
    if (r_lo < r_hi) {
#pragma unroll
        for (int k = 0; k < KCH; ++k)
            if (QN_HD_IN(k)) cur[k] = QN_HD_LD(a.A + (size_t)r_lo * np, k);
    }
    for (int r = r_lo; r < r_hi; ++r) {
        const double* nrow = a.A + (size_t)((r + 1 < r_hi) ? r + 1 : r) * np; // (last row: a harmless re-read, no branch)
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            nxt[k] = (v2d){0.0, 0.0};
            if (QN_HD_IN(k)) nxt[k] = QN_HD_LD(nrow, k);
        }
        const double pr = pw[a.rank * a.mrpr + r];
        const bool live = pr != 0.0;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const double s0 = cur[k].x * cur[k].x, s1 = cur[k].y * cur[k].y;
            const double t0 = __builtin_fma(pr, s0, g[k].x), t1 = __builtin_fma(pr, s1, g[k].y);
            g[k].x = live ? t0 : g[k].x; // (selects: a masked row adds nothing even where its entries are not finite)
            g[k].y = live ? t1 : g[k].y;
            cur[k] = nxt[k];
        }
    }
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int j = 2 * tid + 1024 * k;
        if (j < np) st2(wgg + (size_t)blockIdx.x * np + j, g[k]);
    }
#undef QN_HD_IN
#undef QN_HD_LD
}

// rule 2' of qn_newton_cg.hip.h: what the preconditioned inner loop multiplies by
__device__ __forceinline__ double hd_minv(double m) { return (m > 0.0 && !isinf(m)) ? 1.0 / m : 1.0; }

// 64 columns per workgroup, G <= 256 workgroups' shares: see the head of this file.  minv_out may be NULL
__global__ __launch_bounds__(256) void hd_combine_kernel(const QnLseArgs a, int G, const double* __restrict__ wgg, const double* __restrict__ gbar,
                                                         double* __restrict__ m_out, double* __restrict__ minv_out) {
    __shared__ double part[3][64];
    const int tid = threadIdx.x;
    const int c = tid & 63, q = tid >> 6;
    const int j = min(blockIdx.x * 64 + c, a.n_pad - 1);
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
    if (q != 0) return; // (wave 0 goes on alone: no barrier follows)
    if (blockIdx.x * 64 + c >= a.n_pad) return;
    double mj = 0.0, mi = 1.0;
    if (blockIdx.x * 64 + c < a.n) {
        const double gs = ((acc + part[0][c]) + part[1][c]) + part[2][c];
        const double gb = gbar[j];
        const double gg = gb * gb;
        mj = (gs - gg) + a.mu;
        mi = hd_minv(mj);
    }
    m_out[j] = mj;
    if (minv_out) minv_out[j] = mi;
}

template <int KCH>
static int hd_launch(hipStream_t st, int G, const QnLseArgs& a, const double* pw, double* wgg) {
    // the product's rule: rows of A that cannot stay in the Infinity Cache between passes are requested as non-temporal (QN_LSE_NT = 0 / 1 overrides)
    static const int nt_env = getenv("QN_LSE_NT") ? atoi(getenv("QN_LSE_NT")) : -1;
    const bool nt = nt_env >= 0 ? nt_env != 0 : (size_t)a.mrpr * (size_t)a.n_pad * sizeof(double) > ((size_t)230 << 20);
    if (nt) hipLaunchKernelGGL((hd_onepass_kernel<KCH, true>), dim3(G), dim3(512), 0, st, a, pw, wgg);
    else hipLaunchKernelGGL((hd_onepass_kernel<KCH, false>), dim3(G), dim3(512), 0, st, a, pw, wgg);
    return QN_OK;
}

// enqueue M = diag H(x) into m_dev and, where minv_dev is not NULL, rule 2''s 1 / M into minv_dev (n_pad entries each), with the weights of the
// kind's last weights pass in o->wp.w and its gbar (the table's: lse.gall as lse_enqueue_weights left it, or zeros).  Two launches, unpredicated
static int dense_enqueue_hess_diag(qn_objective* o, double* m_dev, double* minv_dev) {
    QNCHK(lse_hv_built(o));
    hipStream_t st = o->ctx->stream;
    const QnLseArgs a = dense_stream_args(o);
    QNCHK(lse_kch_call(o->os.kch, [&](auto K) { return hd_launch<decltype(K)::value>(st, o->os.G, a, o->wp.w, o->os.wgg); }));
    hipLaunchKernelGGL(hd_combine_kernel, dim3((a.n_pad + 63) / 64), dim3(256), 0, st, a, o->os.G, (const double*)o->os.wgg, o->ops->gbar(o), m_dev, minv_dev);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// diag H(x) of any kind that has one: the weights at x, then the diagonal pass, n entries downloaded
extern "C" int qn_objective_hess_diag_at(qn_objective* o, const double* x_host, double* diag_host) {
    if (!o || !x_host || !diag_host) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    const QnObjOps* ops = o->ops;
    if (!ops->hess_diag) return fail(QN_ERROR_INPUT_PARAMS, "qn_objective_hess_diag_at: not built for this objective (LogSumExp, Logistic and SparseLogistic have a Hessian diagonal)");
    if (ops->hv_built) QNCHK(ops->hv_built(o));
    qn_context* c = o->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t np = o->T.n_pad;
    QNCHK(o->ex.ensure(2 * np, c->stream));
    QNCHK(o->eg.ensure(np, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(ops->weights(o, o->ex));
    QNCHK(ops->hess_diag(o, o->eg, nullptr));
    HIPCHK(hipMemcpyAsync(diag_host, o->eg, o->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return QN_OK;
}
