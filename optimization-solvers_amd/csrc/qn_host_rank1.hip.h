// qn_host_rank1.hip.h -- host side of Broyden / BroydenB (QN_BROYDEN): the launches of csrc/qn_rank1.hip.h.  The solver runs on the generic
// control-step machine with synchronous requests; a QN_PH_REQ_HPASS of that machine is met here by ONE pass over the full, non-symmetric H
// (r1_pass_kernel) and its fixed-order second stage (r1_reduce_kernel), which leave u = H y (and v = H g+) where the machine reads the
// generic pass's row sums, and w = H' s in the pending update's `up`.
#pragma once

static int r1_alloc(qn_solver* s) {
    const int nb = (s->T.n_pad + QN_R1_TB - 1) / QN_R1_TB;
    QNCHK(s->r1_part.ensure((size_t)3 * nb * s->T.n_pad, s->ctx->stream)); // row partials [2][nb][n_pad], column partials [nb][n_pad]
    s->r1_nb = nb;
    return QN_OK;
}

// one pass: the pending update (if any) applied and written back, `nrhs` row sums against r0 / r1, column sums against scol (if not null)
static int r1_launch(qn_solver* s, bool pending, double c, int nrhs, const double* r0, const double* r1, const double* scol) {
    QNCHK(r1_alloc(s));
    hipStream_t st = s->ctx->stream;
    QnR1Args a{};
    a.H = s->H; a.n = (int)s->n; a.n_pad = s->T.n_pad; a.nb = s->r1_nb;
    a.a = s->V.sp; a.w = s->V.up; a.c = c;
    a.r0 = r0; a.r1 = r1; a.scol = scol;
    a.rowpart = s->r1_part; a.colpart = s->r1_part + (size_t)2 * a.nb * a.n_pad;
    a.hp = s->V.hp; a.wout = s->V.up;
    a.nrhs = nrhs; a.col = scol ? 1 : 0;
    const dim3 grid(a.nb, a.nb), blk(256);
    {
        ProfScope ps(s, KC_HPASS);
        const int key = nrhs * 4 + (pending ? 2 : 0) + (scol ? 1 : 0);
        switch (key) {
        case 2: hipLaunchKernelGGL((r1_pass_kernel<0, true, false>), grid, blk, 0, st, a); break;  // flush
        case 4: hipLaunchKernelGGL((r1_pass_kernel<1, false, false>), grid, blk, 0, st, a); break; // direction
        case 6: hipLaunchKernelGGL((r1_pass_kernel<1, true, false>), grid, blk, 0, st, a); break;
        case 5: hipLaunchKernelGGL((r1_pass_kernel<1, false, true>), grid, blk, 0, st, a); break;  // update: u, w
        case 7: hipLaunchKernelGGL((r1_pass_kernel<1, true, true>), grid, blk, 0, st, a); break;
        case 9: hipLaunchKernelGGL((r1_pass_kernel<2, false, true>), grid, blk, 0, st, a); break;  // update: u, v, w
        case 11: hipLaunchKernelGGL((r1_pass_kernel<2, true, true>), grid, blk, 0, st, a); break;
        default: return fail(QN_ABNORMAL_TERMINATION, "rank-1 pass: no such instance");
        }
        s->stats.launches++;
        HIPCHK(hipGetLastError());
    }
    if (nrhs > 0 || scol) {
        ProfScope ps(s, KC_HREDUCE);
        hipLaunchKernelGGL(r1_reduce_kernel, dim3((a.n_pad + 255) / 256), blk, 0, st, a);
        s->stats.launches++;
        HIPCHK(hipGetLastError());
    }
    return QN_OK;
}

// H_stored <- H_true (the caller clears QnCtl.pending)
static int r1_flush(qn_solver* s) { return r1_launch(s, true, s->hctl->c_ss, 0, nullptr, nullptr, nullptr); }

// the machine's QN_PH_REQ_HPASS (the host has just read the control block): a direction pass (d = -H g, broyden.rs:47) or an update pass
static int r1_enqueue_req(qn_solver* s) {
    const QnCtl* h = s->hctl;
    const bool pending = h->pending != 0;
    if (h->after_state == QN_ST_AFTER_DIR) return r1_launch(s, pending, h->c_ss, 1, s->V.g, nullptr, nullptr);
    return r1_launch(s, pending, h->c_ss, h->hp_nrhs == 2 ? 2 : 1, s->V.y, s->V.g, s->V.s);
}

// qn_solver_secant_update for Broyden (the norms are recorded, the skip rule has passed, nothing is pending): the update pass on (s, y), then the
// pending update it leaves applied at once
static int r1_secant_update(qn_solver* s, const double* s_host, const double* y_host, double ys) {
    qn_context* c = s->ctx;
    const size_t n = s->n, np = s->T.n_pad;
    HIPCHK(hipMemcpyAsync(s->V.s, s_host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->V.y, y_host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    QNCHK(r1_launch(s, false, 0.0, 1, s->V.y, nullptr, s->V.s)); // u = H y -> hp, w = H' s -> up
    std::vector<double> a(np, 0.0);
    HIPCHK(hipMemcpyAsync(a.data(), s->V.hp, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) a[i] = s_host[i] - a[i]; // a = s - H y
    HIPCHK(hipMemcpyAsync(s->V.sp, a.data(), np * sizeof(double), hipMemcpyHostToDevice, c->stream));
    s->hctl->c_ss = 1.0 / ys; s->hctl->c_su = 0.0; s->hctl->c_uu = 0.0;
    QNCHK(r1_flush(s));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->hctl->pending = 0;
    return poke_ctl(s);
}
