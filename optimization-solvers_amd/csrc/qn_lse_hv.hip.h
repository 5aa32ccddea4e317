// qn_lse_hv.hip.h -- the Hessian-vector product of the log-sum-exp objective, q = H v with H = A'(diag(p) - p p')A + mu I, without the matrix:
//
//     H v = A'(p o (A v)) - gbar (p . (A v)) + mu v,      p = softmax(A x + c),  gbar = A'p
//
// ONE stream of A (8 m n bytes, what one evaluation moves) where the dense Hessian (qn_lse_hess.hip.h) costs O(m n^2) flops and 8 n^2 bytes.
// p and gbar are what lse_enqueue_weights leaves in `wp.w` and `lse.gall` at x (two passes of A, once per point x; any number of products follow).
//
//   lse_hv_onepass_kernel<KCH, NTA>   lse_onepass_kernel's sibling (qn_kernels.hip.h): its geometry (512 threads, the same row cut over os.G
//                                     workgroups), v staged in LDS where that kernel stages x, each thread's KCH x 2 columns of the current and of
//                                     the prefetched row in registers, ONE barrier per row for u_r = a_r . v in that kernel's order (FMA chain per
//                                     thread, wave butterfly, eight partials added in index order), the same non-temporal rule for A.  No exp, no
//                                     running maximum, no rescale: w_r = p_r u_r (one rounding), G += w_r a_r (FMA), S += w_r.  A row with p_r = 0
//                                     (masked, padding) adds nothing: w_r is then 0 by a select, whatever u_r is.  Each workgroup writes (S, G); one
//                                     that owns no row writes zeros.
//   lse_hv_combine_kernel             q_j = (sum_wg G_wg,j in lse_combine_kernel's order: each quarter of the workgroups in workgroup order, sixteen
//                                     loads in flight, the quarters added in order) - (sum_wg S_wg) gbar_j + mu v_j, the two products rounded on
//                                     their own; and the workgroup's share of sum_j v_j q_j (product and sum round separately, wave butterfly over
//                                     its 64 columns).  The shares are added in index order by whoever consumes them
//                                     (lse_hv_sum_shares: thread b holds share b, wave butterfly, the waves in order -- the family's convention).
//   lse_hv_shares_kernel              (1 workgroup) that consumer for the stand-alone entry; QN_NEWTON_CG's is tn_step_kernel (qn_newton_cg.hip.h).
// Both kernels take a `const QnVecCtl*`: non-null, they return at once unless QN_NEWTON_CG's inner loop is running; null, they always run.
//
// No atomics, no workgroup waits for another, every order is fixed: the same bits for the same (x, v) from run to run and from object to object.
// Built for n_pad <= 16384 -- where the one-pass evaluation exists (os.kch != 0) -- and on one rank.
#pragma once

template <int KCH, bool NTA>
__global__ __launch_bounds__(512) void lse_hv_onepass_kernel(const QnLseArgs a, const double* __restrict__ v, const double* __restrict__ pw,
                                                             double* __restrict__ wgs, double* __restrict__ wgg, const QnVecCtl* __restrict__ ctl) {
    extern __shared__ __attribute__((aligned(16))) double lse_v[]; // KCH * 1024 entries of v, zero past n
    __shared__ double red[2][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = a.n_pad;
    if (ctl && (ctl->phase != QN_VP_NSOLVE || ctl->method != QN_NEWTON_CG || ctl->tn_state != QN_TN_RUNNING)) return;
    // column pair k of this thread: 2 tid + 1024 k.  Past the end NOTHING is loaded (the pair stays zero; its G entries are never stored): a
    // predicated load per chunk where lse_onepass_kernel clamps the column -- sixteen clamped offsets are sixteen live registers, the predicate
    // is a mask in scalar registers, and at KCH = 16 that is the difference between 256 registers with 9 spilled and 240 with none
#define QN_LSE_IN(k) (2 * tid + 1024 * (k) < np)
#define QN_LSE_LD(row, k) (NTA ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>((row) + 1024 * (k) + 2 * tid)) : ld2((row) + 1024 * (k) + 2 * tid))
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int j = 2 * tid + 1024 * k;
        v2d xv = {0.0, 0.0};
        if (j < np) xv = ld2(v + j);
        lse_v[j] = j < a.n ? xv.x : 0.0; lse_v[j + 1] = j + 1 < a.n ? xv.y : 0.0;
    }
    __syncthreads();
    const int G = gridDim.x, per = (a.mrpr + G - 1) / G;
    const int r_lo = blockIdx.x * per;
    const int r_hi = min(min(a.mrpr, r_lo + per), a.m - a.rank * a.mrpr); // (rows past m are padding)
    v2d g[KCH], cur[KCH], nxt[KCH];
#pragma unroll
    for (int k = 0; k < KCH; ++k) { g[k] = (v2d){0.0, 0.0}; cur[k] = (v2d){0.0, 0.0}; }
    double s_run = 0.0;
    if (r_lo < r_hi) {
#pragma unroll
        for (int k = 0; k < KCH; ++k)
            if (QN_LSE_IN(k)) cur[k] = QN_LSE_LD(a.A + (size_t)r_lo * np, k);
    }
    for (int r = r_lo; r < r_hi; ++r) {
        const double* nrow = a.A + (size_t)((r + 1 < r_hi) ? r + 1 : r) * np; // (last row: a harmless re-read, no branch)
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            nxt[k] = (v2d){0.0, 0.0};
            if (QN_LSE_IN(k)) nxt[k] = QN_LSE_LD(nrow, k);
        }
        const double pr = pw[a.rank * a.mrpr + r];
        double p = 0.0;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const int j = 2 * tid + 1024 * k;
            const v2d xv = *reinterpret_cast<const v2d*>(&lse_v[j]);
            p = __builtin_fma(cur[k].x, xv.x, p);
            p = __builtin_fma(cur[k].y, xv.y, p);
        }
        p = qn_wave_sum(p);
        if (lane == 0) red[r & 1][wave] = p;
        __syncthreads();
        double u = red[r & 1][0];
#pragma unroll
        for (int w = 1; w < 8; ++w) u = u + red[r & 1][w];
        const double pu = pr * u;
        const double wr = pr == 0.0 ? 0.0 : pu; // (a select, not a branch: a masked row adds nothing even where its u is not finite)
        s_run = s_run + wr;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            g[k].x = __builtin_fma(wr, cur[k].x, g[k].x);
            g[k].y = __builtin_fma(wr, cur[k].y, g[k].y);
            cur[k] = nxt[k];
        }
    }
    if (tid == 0) wgs[blockIdx.x] = s_run;
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int j = 2 * tid + 1024 * k;
        if (j < np) st2(wgg + (size_t)blockIdx.x * np + j, g[k]);
    }
#undef QN_LSE_IN
#undef QN_LSE_LD
}

// 64 columns per workgroup, G <= 256 workgroups' results: see the head of this file
__global__ __launch_bounds__(256) void lse_hv_combine_kernel(const QnLseArgs a, int G, const double* __restrict__ wgs, const double* __restrict__ wgg,
                                                             const double* __restrict__ v, const double* __restrict__ gbar, double* __restrict__ q_out,
                                                             double* __restrict__ shares, const QnVecCtl* __restrict__ ctl) {
    __shared__ double lds[16];
    __shared__ double part[3][64];
    if (ctl && (ctl->phase != QN_VP_NSOLVE || ctl->method != QN_NEWTON_CG || ctl->tn_state != QN_TN_RUNNING)) return;
    const int tid = threadIdx.x;
    double s[1] = {tid < G ? wgs[tid] : 0.0}; // sum_wg S_wg: thread w holds workgroup w's; wave butterfly, then the four waves in order
    ctl_block_sum<1>(s, lds);
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
    const bool live = blockIdx.x * 64 + c < a.n;
    double vq = 0.0;
    if (live) {
        const double gs = ((acc + part[0][c]) + part[1][c]) + part[2][c];
        const double vj = v[j];
        const double sg = s[0] * gbar[j];
        const double mv = a.mu * vj;
        const double qj = (gs - sg) + mv;
        q_out[j] = qj;
        vq = vj * qj;
    } else if (blockIdx.x * 64 + c < a.n_pad) {
        q_out[j] = 0.0;
    }
    vq = qn_wave_sum(vq);
    if (c == 0) shares[blockIdx.x] = vq;
}

// the shares of sum_j v_j q_j (count <= 256), added as every consumer adds them: thread b holds share b, wave butterfly, then the four waves in order
__device__ __forceinline__ double lse_hv_sum_shares(const double* __restrict__ shares, int count, double* lds /* 16 */) {
    double t[1] = {(int)threadIdx.x < count ? shares[threadIdx.x] : 0.0};
    ctl_block_sum<1>(t, lds);
    return t[0];
}
__global__ __launch_bounds__(256) void lse_hv_shares_kernel(const double* __restrict__ shares, int count, double* __restrict__ out) {
    __shared__ double lds[16];
    const double t = lse_hv_sum_shares(shares, count, lds);
    if (threadIdx.x == 0) *out = t;
}

template <int KCH, bool NTA>
static int lse_hv_launch_nt(hipStream_t st, int G, const QnLseArgs& a, const double* v, const double* pw, double* wgs, double* wgg, const QnVecCtl* ctl) {
    static std::atomic<bool> attr_set[64]; // per device, as lse_launch_onepass_nt
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t lds = (size_t)KCH * 1024 * sizeof(double);
    if ((dev < 0 || dev >= 64 || !attr_set[dev].load()) && lds > 48 * 1024) {
        if (hipFuncSetAttribute((const void*)lse_hv_onepass_kernel<KCH, NTA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return fail(QN_ERROR_INPUT_PARAMS, "the log-sum-exp Hessian-vector product is not built for this device: it does not grant the LDS that holds v");
        }
        if (dev >= 0 && dev < 64) attr_set[dev].store(true);
    }
    hipLaunchKernelGGL((lse_hv_onepass_kernel<KCH, NTA>), dim3(G), dim3(512), lds, st, a, v, pw, wgs, wgg, ctl);
    return QN_OK;
}
template <int KCH>
static int lse_hv_launch(hipStream_t st, int G, const QnLseArgs& a, const double* v, const double* pw, double* wgs, double* wgg, const QnVecCtl* ctl) {
    // the evaluation's rule: rows of A that cannot stay in the Infinity Cache between passes are requested as non-temporal (QN_LSE_NT = 0 / 1 overrides)
    static const int nt_env = getenv("QN_LSE_NT") ? atoi(getenv("QN_LSE_NT")) : -1;
    const bool nt = nt_env >= 0 ? nt_env != 0 : (size_t)a.mrpr * (size_t)a.n_pad * sizeof(double) > ((size_t)230 << 20);
    return nt ? lse_hv_launch_nt<KCH, true>(st, G, a, v, pw, wgs, wgg, ctl) : lse_hv_launch_nt<KCH, false>(st, G, a, v, pw, wgs, wgg, ctl);
}

// what the one-rank kernels of the dense kinds read of QnLseArgs: A, mu and the shapes (the multinomial's: the flat vector of N entries in N_pad)
static QnLseArgs dense_stream_args(const qn_objective* o) {
    QnLseArgs a{};
    a.A = o->dn.rows; a.mu = o->dn.mu;
    a.m = (int)o->dn.m; a.m_pad = o->dn.TA.n_pad; a.mrpr = o->dn.TA.rpr; a.n = (int)o->n; a.n_pad = o->T.n_pad;
    a.world = 1; a.rank = 0; a.rs = 1;
    return a;
}

static int lse_hv_built(const qn_objective* o) {
    if (o->ctx->world != 1) return fail(QN_ERROR_INPUT_PARAMS, "the log-sum-exp Hessian-vector product is single-GPU (not built for a row-sharded context)");
    if (!o->os.kch) return fail(QN_ERROR_INPUT_PARAMS, "the log-sum-exp Hessian-vector product is not built for n_pad > 16384 (it exists where the one-pass evaluation does)");
    return QN_OK;
}

// enqueue q = H v into q_dev (n_pad entries, zero past n) and the shares of v'Hv into o->os.hv_shares, with p in o->wp.w and gbar in gbar_dev
// (o->lse.gall after lse_enqueue_weights at the point x; QN_NEWTON_CG keeps a copy, an evaluation in between overwrites it).  v_dev: n_pad entries.
// The evaluation's per-workgroup scratch is reused: one stream, and every evaluation rewrites all of it.  `ctl` != NULL (QN_NEWTON_CG's inner
// loop): both launches return at once unless the control block says that loop is running; NULL (qn_objective_hess_vec_at): unconditional --
// spq_curv_kernel's pattern.  `which`: 1 the stream of A, 2 the combine, 3 both (profiling mode times the two apart).
static int lse_enqueue_hess_vec(qn_objective* o, const double* v_dev, const double* gbar_dev, double* q_dev, const QnVecCtl* ctl, int which) {
    QNCHK(lse_hv_built(o));
    hipStream_t st = o->ctx->stream;
    const int np = o->T.n_pad;
    QNCHK(o->os.hv_shares.ensure(257, st));
    const QnLseArgs a = dense_stream_args(o);
    int lst = QN_OK;
    if (which & 1) lst = lse_kch_call(o->os.kch, [&](auto K) { return lse_hv_launch<decltype(K)::value>(st, o->os.G, a, v_dev, o->wp.w, o->os.wgms, o->os.wgg, ctl); });
    QNCHK(lst);
    if (which & 2)
        hipLaunchKernelGGL(lse_hv_combine_kernel, dim3((np + 63) / 64), dim3(256), 0, st, a, o->os.G, (const double*)o->os.wgms, (const double*)o->os.wgg, v_dev,
                           gbar_dev, q_dev, (double*)o->os.hv_shares, ctl);
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// ---- what the kinds that share these kernels (LogSumExp, Logistic, Multinomial) put into their tables ----
// v'Hv: the combine kernel's shares, one per 64 columns
static int lse_hv_out(qn_objective* o, QnHvOut* out) {
    QNCHK(o->os.hv_shares.ensure(257, o->ctx->stream));
    *out = QnHvOut{o->os.hv_shares, (o->T.n_pad + 63) / 64, true};
    return QN_OK;
}
// H = A' diag(d) A + mu I (the logistic pair, the multinomial): zeros where log-sum-exp has gbar
static const double* wp_zero_gbar(const qn_objective* o) { return o->wp.zero; }
// qn_stats.obj_bytes: one stream of the dense A (a product; the logistic's evaluation and weights pass)
static uint64_t dense_stream_bytes(const qn_objective* o) { return (uint64_t)o->dn.m * (uint64_t)o->T.n_pad * 8ull; }

static int lse_weights_op(qn_objective* o, const double* x_dev) { QnLseArgs a{}; return lse_enqueue_weights(o, x_dev, a); } // p -> wp.w, gbar -> lse.gall
static const double* lse_gbar(const qn_objective* o) { return o->lse.gall; }
// one pass over this rank's rows of A per evaluation (two for n > 16384), as the dense family counts it
static uint64_t lse_eval_bytes(const qn_objective* o) {
    return (uint64_t)o->dn.TA.rpr * (uint64_t)o->T.n_pad * 8ull * ((o->os.kch && !o->lse.two_pass) ? 1ull : 2ull);
}
static uint64_t lse_weights_bytes(const qn_objective* o) { return 2ull * dense_stream_bytes(o); }

static const QnObjOps kLseOps = {
    /* eval */ lse_enqueue_eval, /* eval_launches */ 0, /* eval_split */ false, /* vec_counted */ false,
    /* weights */ lse_weights_op, 4,
    /* hv_built, hess_vec, gbar, hv_out */ lse_hv_built, lse_enqueue_hess_vec, lse_gbar, lse_hv_out, 2, false,
    /* curvature, curv_shares; hessian */ nullptr, nullptr, lse_enqueue_hessian, 5,
    /* bytes: eval, product, weights, curvature */ lse_eval_bytes, dense_stream_bytes, lse_weights_bytes, nullptr,
    /* no_dense_family */ nullptr, /* no_rows */ nullptr, /* no_hessian */ nullptr,
    /* no_curvature */ "qn_objective_hess_vec: not built for this objective (a dense or a sparse quadratic has a Hessian-vector product)",
    /* hess_diag, its launches and bytes */ dense_enqueue_hess_diag, 2, dense_stream_bytes,
};
static const QnObjOps* lse_ops() { return &kLseOps; }

// (H(x) v, v'H(x)v) of any kind: the weights at x, one product, the shares' sum where the kind leaves shares.  A quadratic's Hessian is Q: x is not read
extern "C" int qn_objective_hess_vec_at(qn_objective* o, const double* x_host, const double* v_host, double* q_host, double* vhv) {
    if (!o || !v_host || !vhv) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    const QnObjOps* ops = o->ops;
    if (ops->curvature) return qn_objective_hess_vec(o, v_host, q_host, vhv);
    if (!x_host) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (ops->hv_built) QNCHK(ops->hv_built(o));
    qn_context* c = o->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t np = o->T.n_pad;
    QNCHK(o->ex.ensure(2 * np, c->stream)); // x, then v
    QNCHK(o->eg.ensure(np, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex, x_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(o->ex + np, v_host, o->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(ops->weights(o, o->ex));
    QNCHK(ops->hess_vec(o, o->ex + np, ops->gbar(o), o->eg, nullptr, 3));
    QnHvOut out{};
    QNCHK(ops->hv_out(o, &out));
    if (out.sum) {
        hipLaunchKernelGGL(lse_hv_shares_kernel, dim3(1), dim3(256), 0, c->stream, out.shares, out.count, (double*)out.shares + 256);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(vhv, out.sum ? out.shares + 256 : out.shares, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (q_host) HIPCHK(hipMemcpyAsync(q_host, o->eg, o->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return QN_OK;
}
