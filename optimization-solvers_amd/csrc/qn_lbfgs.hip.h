// qn_lbfgs.hip.h -- limited-memory BFGS (QN_LBFGS; ProjectedLBFGS once qn_solver_set_bounds is called) on the first-order family's machine
// (qn_vec.hip.h): phase QN_VP_NSOLVE with z = H_k g formed from the last k <= m pairs (s, y) where projected Newton has z = H^-1 g.
// NOT the Fortran L-BFGS-B algorithm (no generalised Cauchy point, no subspace minimisation): the bounded variant is this project's BFGSB
// convention, d = P(x - H g) - x (bfgs_b.rs:72-75).
//
// The direction is the COMPACT FORM of Byrd, Nocedal and Schnabel (1994) and not the two-loop recursion (2 m dependent device-wide reductions):
// with the pairs ordered oldest to newest, R = triu(S'Y), D = diag(s_i.y_i), gamma = s_k.y_k / y_k.y_k, p = S'g, q = Y'g,
//     v = -R^-1 p,   u = R^-T [(D + gamma Y'Y) R^-1 p - gamma q],   z = gamma g + S u + gamma Y v.
//
//   lbfgs_gram_kernel    ONE stream of S, Y and g: per-workgroup shares of S_j.g, Y_j.g, S_j.y_p, s_p.Y_j, Y_j.y_p for every stored pair j
//                        ((s_p, y_p): the newest pair) and of g.g -- 5 k + 1 sums, (2 k + 1) 8 n bytes.  grid (vec_grid, ceil(k / 4)): a
//                        workgroup holds the 20 accumulators of 4 pairs; g, s_p, y_p are read again by every group, out of L2.
//   lbfgs_mid_kernel     (1 workgroup) adds the shares in index order, refreshes row and column p of the small Gram matrices S'Y and Y'Y, the two
//                        triangular solves with R (k <= 32, one thread), the safeguard g.z = gamma g.g + u.p + gamma v.q > 0
//   lbfgs_apply_kernel   the second stream: z = gamma g + sum_j (u_j S_j + gamma v_j Y_j), oldest to newest, per element in that order
//   lbfgs_accept_kernel  vec_accept_kernel for this method: it also stores s and y into the staging slot and leaves y.y
// (vec_post_kernel commits the pair: qn_vec.hip.h.)
//
// SLOTS.  The ring has m + 1 slots of n_pad doubles for S and for Y.  The live pairs are slots head .. head + k - 1 (mod m + 1), oldest first; the
// accept kernel writes into slot head + k (mod m + 1) -- with a full memory that is the slot the oldest pair will vacate next -- and the post
// kernel commits it (k += 1, or head += 1 when k == m) only when s.y > DBL_EPSILON y.y.  A pair that is not committed leaves the memory as it
// was; no vector is ever copied.  The Gram matrices are indexed by SLOT, so a commit refreshes one row and one column and moves nothing.
//
// Reductions as in qn_vec.hip.h: two-stage and fixed (share b of quantity q in lpart[q * QN_VEC_MAXG + b], added in index order), no
// floating-point atomic, no kernel waits for another workgroup; products and sums round twice.  Every kernel is predicated on
// QnVecCtl.phase == QN_VP_NSOLVE (the accept kernel on QN_VP_ACCEPT): the host enqueues them without reading a decision.
#pragma once

#define QN_LBFGS_SLOTS (QN_LBFGS_MAX_M + 1)
#define QN_LBFGS_GROUP 4                    // pairs per workgroup of the Gram kernel
#define QN_LBFGS_NQ (5 * QN_LBFGS_MAX_M + 1) // quantities of the share buffer: 5 per pair (by age), then g.g
// the small block (doubles): S'Y and Y'Y by slot, then what the mid kernel leaves for the apply kernel
#define QN_LB_SY 0
#define QN_LB_YY (QN_LBFGS_SLOTS * QN_LBFGS_SLOTS)
#define QN_LB_U (2 * QN_LBFGS_SLOTS * QN_LBFGS_SLOTS)
#define QN_LB_GV (QN_LB_U + QN_LBFGS_MAX_M)   // gamma v_j
#define QN_LB_GAMMA (QN_LB_GV + QN_LBFGS_MAX_M)
#define QN_LB_K (QN_LB_GAMMA + 1)             // pairs the apply kernel uses (0 after the safeguard)
#define QN_LB_SMALL_LEN (QN_LB_K + 1)

__global__ __launch_bounds__(QN_VEC_TPB) void lbfgs_gram_kernel(const QnVecArgs a) {
    constexpr int NA = 5 * QN_LBFGS_GROUP + 1;
    __shared__ double lds[4 * NA];
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_NSOLVE) return;
    const int k = c->lb_kmem, head = c->lb_head, M = c->lb_m + 1;
    const int i0 = blockIdx.y * QN_LBFGS_GROUP;
    if (i0 >= k && blockIdx.y != 0) return; // (group 0 always runs: g.g)
    const int cnt = min(QN_LBFGS_GROUP, max(0, k - i0));
    const size_t np = (size_t)a.np;
    const int pn = k > 0 ? (head + k - 1) % M : 0;
    const double* sp = a.lS + (size_t)pn * np;
    const double* yp = a.lY + (size_t)pn * np;
    const double *Sj[QN_LBFGS_GROUP], *Yj[QN_LBFGS_GROUP];
#pragma unroll
    for (int u = 0; u < QN_LBFGS_GROUP; ++u) {
        const int slot = u < cnt ? (head + i0 + u) % M : pn;
        Sj[u] = a.lS + (size_t)slot * np;
        Yj[u] = a.lY + (size_t)slot * np;
    }
    double acc[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q) acc[q] = 0.0;
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d g = ld2(a.g + 2 * j);
        v2d s = {0.0, 0.0}, y = {0.0, 0.0};
        if (cnt > 0) { s = ld2(sp + 2 * j); y = ld2(yp + 2 * j); }
#pragma unroll
        for (int u = 0; u < QN_LBFGS_GROUP; ++u) {
            if (u < cnt) {
                const v2d S = ld2(Sj[u] + 2 * j), Y = ld2(Yj[u] + 2 * j);
                acc[5 * u + 0] = acc[5 * u + 0] + S.x * g.x; acc[5 * u + 0] = acc[5 * u + 0] + S.y * g.y;
                acc[5 * u + 1] = acc[5 * u + 1] + Y.x * g.x; acc[5 * u + 1] = acc[5 * u + 1] + Y.y * g.y;
                acc[5 * u + 2] = acc[5 * u + 2] + S.x * y.x; acc[5 * u + 2] = acc[5 * u + 2] + S.y * y.y;
                acc[5 * u + 3] = acc[5 * u + 3] + s.x * Y.x; acc[5 * u + 3] = acc[5 * u + 3] + s.y * Y.y;
                acc[5 * u + 4] = acc[5 * u + 4] + Y.x * y.x; acc[5 * u + 4] = acc[5 * u + 4] + Y.y * y.y;
            }
        }
        acc[NA - 1] = acc[NA - 1] + g.x * g.x;
        acc[NA - 1] = acc[NA - 1] + g.y * g.y;
    }
    ctl_block_sum<NA>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int u = 0; u < QN_LBFGS_GROUP; ++u) {
            if (u < cnt) {
#pragma unroll
                for (int t = 0; t < 5; ++t) a.lpart[(size_t)(5 * (i0 + u) + t) * QN_VEC_MAXG + blockIdx.x] = acc[5 * u + t];
            }
        }
        if (blockIdx.y == 0) a.lpart[(size_t)(QN_LBFGS_NQ - 1) * QN_VEC_MAXG + blockIdx.x] = acc[NA - 1];
    }
}

__global__ __launch_bounds__(QN_VEC_TPB) void lbfgs_mid_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    __shared__ double P[5][QN_LBFGS_MAX_M]; // by age: S_i.g, Y_i.g, S_i.y_p, s_p.Y_i, Y_i.y_p
    __shared__ double GG;
    __shared__ double R[QN_LBFGS_MAX_M][QN_LBFGS_MAX_M + 1], W[QN_LBFGS_MAX_M][QN_LBFGS_MAX_M + 1]; // S'Y and Y'Y by age
    __shared__ double w[QN_LBFGS_MAX_M], rr[QN_LBFGS_MAX_M], uu[QN_LBFGS_MAX_M];
    QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_NSOLVE) return;
    const int k = c->lb_kmem, head = c->lb_head, M = c->lb_m + 1;
    const int tid = threadIdx.x;
    double* sm = a.lsmall;
    for (int i = 0; i < k; ++i) {
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int b = tid; b < a.G; b += QN_VEC_TPB) {
#pragma unroll
            for (int t = 0; t < 5; ++t) v[t] = v[t] + a.lpart[(size_t)(5 * i + t) * QN_VEC_MAXG + b];
        }
        __syncthreads();
        ctl_block_sum<5>(v, lds);
        if (tid == 0) {
#pragma unroll
            for (int t = 0; t < 5; ++t) P[t][i] = v[t];
        }
    }
    {
        double v[1] = {0.0};
        for (int b = tid; b < a.G; b += QN_VEC_TPB) v[0] = v[0] + a.lpart[(size_t)(QN_LBFGS_NQ - 1) * QN_VEC_MAXG + b];
        __syncthreads();
        ctl_block_sum<1>(v, lds);
        if (tid == 0) GG = v[0];
    }
    for (int e = tid; e < k * k; e += QN_VEC_TPB) {
        const int i = e / k, j = e % k;
        const int si = (head + i) % M, sj = (head + j) % M;
        R[i][j] = sm[QN_LB_SY + si * QN_LBFGS_SLOTS + sj];
        W[i][j] = sm[QN_LB_YY + si * QN_LBFGS_SLOTS + sj];
    }
    __syncthreads();
    // row and column of the newest pair (the post kernel committed it; the same values again when it is in them already)
    if (tid < k) {
        const int i = tid, p = k - 1;
        const int si = (head + i) % M, spn = (head + p) % M;
        R[i][p] = P[2][i]; R[p][i] = P[3][i];
        W[i][p] = P[4][i]; W[p][i] = P[4][i];
        sm[QN_LB_SY + si * QN_LBFGS_SLOTS + spn] = P[2][i];
        sm[QN_LB_SY + spn * QN_LBFGS_SLOTS + si] = P[3][i];
        sm[QN_LB_YY + si * QN_LBFGS_SLOTS + spn] = P[4][i];
        sm[QN_LB_YY + spn * QN_LBFGS_SLOTS + si] = P[4][i];
    }
    __syncthreads();
    if (tid != 0) return;
    double gamma = 1.0;
    int keff = k;
    if (k > 0) {
        if (!c->lb_unit) gamma = R[k - 1][k - 1] / W[k - 1][k - 1];
        for (int i = k - 1; i >= 0; --i) { // w = R^-1 p
            double acc = P[0][i];
            for (int j = i + 1; j < k; ++j) acc = acc - R[i][j] * w[j];
            w[i] = acc / R[i][i];
        }
        for (int i = 0; i < k; ++i) { // (D + gamma Y'Y) w - gamma q
            double yw = 0.0;
            for (int j = 0; j < k; ++j) yw = yw + W[i][j] * w[j];
            rr[i] = (R[i][i] * w[i] + gamma * yw) - gamma * P[1][i];
        }
        for (int i = 0; i < k; ++i) { // u = R^-T (.)
            double acc = rr[i];
            for (int j = 0; j < i; ++j) acc = acc - R[j][i] * uu[j];
            uu[i] = acc / R[i][i];
        }
        double up = 0.0, vq = 0.0;
        for (int i = 0; i < k; ++i) up = up + uu[i] * P[0][i];
        for (int i = 0; i < k; ++i) vq = vq - w[i] * P[1][i];
        const double gz = (gamma * GG + up) + gamma * vq;
        if (!(gz > 0.0) || isinf(gz)) { // not a descent direction (or not a number): the memory is cleared and z = g
            keff = 0; gamma = 1.0;
            c->lb_kmem = 0; c->lb_head = 0; c->lb_resets++;
        }
    }
    for (int i = 0; i < keff; ++i) { sm[QN_LB_U + i] = uu[i]; sm[QN_LB_GV + i] = gamma * (-w[i]); }
    sm[QN_LB_GAMMA] = gamma;
    sm[QN_LB_K] = (double)keff;
    c->lb_gamma = gamma;
}

__global__ __launch_bounds__(QN_VEC_TPB) void lbfgs_apply_kernel(const QnVecArgs a) {
    __shared__ double cu[QN_LBFGS_MAX_M], cv[QN_LBFGS_MAX_M];
    __shared__ size_t off[QN_LBFGS_MAX_M];
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_NSOLVE) return;
    const double* sm = a.lsmall;
    const int k = (int)sm[QN_LB_K], head = c->lb_head, M = c->lb_m + 1;
    const double gamma = sm[QN_LB_GAMMA];
    if ((int)threadIdx.x < k) {
        cu[threadIdx.x] = sm[QN_LB_U + threadIdx.x];
        cv[threadIdx.x] = sm[QN_LB_GV + threadIdx.x];
        off[threadIdx.x] = (size_t)((head + (int)threadIdx.x) % M) * (size_t)a.np;
    }
    __syncthreads();
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d g = ld2(a.g + 2 * j);
        v2d z = g; // (no pair: z = g itself)
        if (k > 0) { z.x = gamma * g.x; z.y = gamma * g.y; }
#pragma unroll 4
        for (int i = 0; i < k; ++i) {
            const v2d S = ld2(a.lS + off[i] + 2 * j), Y = ld2(a.lY + off[i] + 2 * j);
            z.x = z.x + cu[i] * S.x; z.y = z.y + cu[i] * S.y;
            z.x = z.x + cv[i] * Y.x; z.y = z.y + cv[i] * Y.y;
        }
        st2(a.zw + 2 * j, z);
    }
}

// vec_accept_kernel for QN_LBFGS: x_next = x + t d, s = x_next - x, y = g(x_next) - g(x) -- stored into the staging slot -- with the shares of
// s.y, s.s and y.y; x <- x_next, g <- g(x_next).  (The machine's vec_needs_y rule has evaluated x_next: gt_valid is set whenever this runs.)
__global__ __launch_bounds__(QN_VEC_TPB) void lbfgs_accept_kernel(const QnVecArgs a) {
    __shared__ double lds[64];
    const QnVecCtl* c = a.ctl;
    if (c->phase != QN_VP_ACCEPT) return;
    const double t = c->t;
    const int64_t row = (int64_t)c->n_iter;
    const bool xtr = c->trace_x && a.xtrace && row < c->trace_cap;
    const int M = c->lb_m + 1;
    const size_t stage = (size_t)((c->lb_head + c->lb_kmem) % M) * (size_t)a.np;
    double* Ss = a.lS + stage;
    double* Ys = a.lY + stage;
    double acc[3] = {0.0, 0.0, 0.0};
    const int nv = a.np >> 1;
    for (int j = blockIdx.x * QN_VEC_TPB + threadIdx.x; j < nv; j += a.G * QN_VEC_TPB) {
        const v2d x = ld2(a.x + 2 * j), d = ld2(a.d + 2 * j);
        const v2d g = ld2(a.g + 2 * j), gt = ld2(a.gt + 2 * j);
        const double td0 = t * d.x, td1 = t * d.y;
        v2d xn, s, y;
        xn.x = x.x + td0;
        xn.y = x.y + td1;
        s.x = xn.x - x.x; s.y = xn.y - x.y;
        y.x = gt.x - g.x; y.y = gt.y - g.y;
        acc[1] = acc[1] + s.x * s.x;
        acc[1] = acc[1] + s.y * s.y;
        acc[0] = acc[0] + s.x * y.x;
        acc[0] = acc[0] + s.y * y.y;
        acc[2] = acc[2] + y.x * y.x;
        acc[2] = acc[2] + y.y * y.y;
        st2(Ss + 2 * j, s);
        st2(Ys + 2 * j, y);
        st2(a.g + 2 * j, gt);
        st2(a.x + 2 * j, xn);
        if (xtr) {
            if (2 * j < a.n) a.xtrace[(size_t)row * a.n + 2 * j] = xn.x;
            if (2 * j + 1 < a.n) a.xtrace[(size_t)row * a.n + 2 * j + 1] = xn.y;
        }
    }
    ctl_block_sum<3>(acc, lds);
    if (threadIdx.x == 0) {
        a.part[2 * QN_VEC_MAXG + blockIdx.x] = acc[0];
        a.part[3 * QN_VEC_MAXG + blockIdx.x] = acc[1];
        a.part[5 * QN_VEC_MAXG + blockIdx.x] = acc[2];
    }
}
