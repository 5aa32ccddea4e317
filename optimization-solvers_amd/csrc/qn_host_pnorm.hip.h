// qn_host_pnorm.hip.h -- host side of PnormDescent / CoordinateDescent (QN_PNORM_DESCENT, QN_COORDINATE_DESCENT): the launches of
// csrc/qn_pnorm.hip.h.  Both solvers run on the generic control-step machine with synchronous requests, beside GradientDescent (the default
// hook x += t d, the ||g||_inf test) and Newton (a direction that arrives from outside the control kernel): a QN_PH_REQ_STEEP of that machine is met
// here by ONE launch -- pnorm_dir_kernel (d, and the shares of g.d, ||g||_inf) or cd_argmax_kernel (the (magnitude, index) shares) -- and the
// machine's QN_ST_AFTER_STEEP folds the shares.  inverse_p is a constructor argument of the reference (pnorm_descent.rs:20): it lives in a buffer
// of its own, row-major and padded like H, survives qn_solver_reset and is never written by a kernel.
#pragma once

static bool steep_method(int method) { return method == QN_COORDINATE_DESCENT || method == QN_PNORM_DESCENT; }

// the shares' buffer and their number: a function of n alone
static int steep_alloc(qn_solver* s) {
    const int np = s->T.n_pad;
    const int ns = s->method == QN_PNORM_DESCENT ? np / QN_PN_SHARE : std::min(1024, (np + QN_CD_SPAN - 1) / QN_CD_SPAN);
    QNCHK(s->steep_part.ensure((size_t)3 * ns, s->ctx->stream));
    s->steep_nshare = ns;
    s->V.steep_part = s->steep_part; s->V.steep_nshare = ns;
    return QN_OK;
}

// WHICH INSTANCE.  Rows per wave: 2 up to n_pad = 8192 (n_pad / 8 workgroups: 512 at n = 4096, two per CU), 4 beyond (n_pad / 16: 1024 at n = 16384).
// Non-temporal loads: the matrix is read once per iteration and by nothing else.  Up to ~230 MB (n ~ 5400) it fits the 256 MB Infinity Cache beside
// the vectors and consecutive iterations find it there -- plain loads keep it; beyond that nothing of it survives an iteration and the stream passes
// the caches by.  The threshold is s2_cache_policy's; the figures behind the default are in DESIGN.md 19.  QN_OPT_PNORM_NONTEMPORAL /
// QN_OPT_PNORM_ROWS_PER_WAVE (and QN_PNORM_NT / QN_PNORM_RW in the environment, for tools/bench_pnorm.py) override; every instance gives the same bits.
static int pnorm_launch(qn_solver* s, const double* g_dev, double* d_dev) {
    QnPnormArgs a{};
    a.P = s->pnorm_P; a.g = g_dev; a.d = d_dev; a.part = s->steep_part;
    a.n = (int)s->n; a.n_pad = s->T.n_pad; a.nshare = s->steep_nshare;
    static const int nt_env = getenv("QN_PNORM_NT") ? atoi(getenv("QN_PNORM_NT")) : -1;
    static const int rw_env = getenv("QN_PNORM_RW") ? atoi(getenv("QN_PNORM_RW")) : 0;
    const int nt_sel = s->pnorm_nt >= 0 ? s->pnorm_nt : nt_env;
    const bool nt = nt_sel >= 0 ? nt_sel != 0 : (size_t)a.n_pad * (size_t)a.n_pad * sizeof(double) > ((size_t)230 << 20);
    int rw = s->pnorm_rw ? s->pnorm_rw : rw_env;
    if (rw != 2 && rw != 4) rw = a.n_pad <= 8192 ? 2 : 4;
    hipStream_t st = s->ctx->stream;
    ProfScope ps(s, KC_HPASS);
    const dim3 grid(a.n_pad / (4 * rw)), blk(QN_PN_TPB);
    if (rw == 2) {
        if (nt) hipLaunchKernelGGL((pnorm_dir_kernel<2, true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((pnorm_dir_kernel<2, false>), grid, blk, 0, st, a);
    } else {
        if (nt) hipLaunchKernelGGL((pnorm_dir_kernel<4, true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((pnorm_dir_kernel<4, false>), grid, blk, 0, st, a);
    }
    s->stats.launches++;
    HIPCHK(hipGetLastError());
    return QN_OK;
}

static int cd_launch(qn_solver* s, const double* g_dev) {
    QnCdArgs a{};
    a.g = g_dev; a.part = s->steep_part; a.n = (int)s->n; a.G = s->steep_nshare;
    a.span = ((s->T.n_pad + a.G - 1) / a.G + 511) / 512 * 512; // contiguous runs, whole 512-index trips
    ProfScope ps(s, KC_HPASS);
    hipLaunchKernelGGL(cd_argmax_kernel, dim3(a.G), dim3(256), 0, s->ctx->stream, a);
    s->stats.launches++;
    HIPCHK(hipGetLastError());
    return QN_OK;
}

// the machine's QN_PH_REQ_STEEP
static int steep_enqueue_req(qn_solver* s) {
    if (s->method == QN_PNORM_DESCENT) return pnorm_launch(s, s->V.g, s->V.d);
    return cd_launch(s, s->V.g);
}

extern "C" int qn_solver_set_inverse_p(qn_solver* s, const double* p) { // PnormDescent::new(grad_tol, x0, inverse_p), pnorm_descent.rs:20-27
    if (!s || !p) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_PNORM_DESCENT) return fail(QN_ERROR_INPUT_PARAMS, "inverse_p belongs to a QN_PNORM_DESCENT solver");
    HIPCHK(hipSetDevice(s->ctx->device));
    const size_t n = s->n, np = s->T.n_pad;
    HIPCHK(hipStreamSynchronize(s->ctx->stream));
    if (!s->pnorm_P) QNCHK(s->pnorm_P.alloc(np * np));
    std::vector<double> rows(np * np, 0.0); // row-major, the padding zero
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) rows[i * np + j] = p[i + j * n]; // column-major in, like DMatrix
    HIPCHK(hipMemcpy(s->pnorm_P, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
    s->pnorm_set = true;
    s->V.H = s->pnorm_P; // (n <= 5: the control kernel's literal column sweep reads it)
    s->hctl->have_dir = 0;
    return poke_ctl(s);
}

extern "C" int qn_solver_get_inverse_p(qn_solver* s, double* out) { // inverse_p(), derive_getters on pnorm_descent.rs:11-17
    if (!s || !out) return fail(QN_ERROR_INPUT_PARAMS, "null argument");
    if (s->method != QN_PNORM_DESCENT) return fail(QN_ERROR_INPUT_PARAMS, "inverse_p belongs to a QN_PNORM_DESCENT solver");
    if (!s->pnorm_set) return fail(QN_ERROR_INPUT_PARAMS, "inverse_p has not been set (qn_solver_set_inverse_p)");
    HIPCHK(hipSetDevice(s->ctx->device));
    const size_t n = s->n, np = s->T.n_pad, chunk = 256;
    std::vector<double> rows(chunk * np);
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t nr = std::min(chunk, n - r0);
        HIPCHK(hipMemcpyAsync(rows.data(), s->pnorm_P + r0 * np, nr * np * sizeof(double), hipMemcpyDeviceToHost, s->ctx->stream));
        HIPCHK(hipStreamSynchronize(s->ctx->stream));
        for (size_t r = 0; r < nr; ++r)
            for (size_t j = 0; j < n; ++j) out[(r0 + r) + j * n] = rows[r * np + j];
    }
    return QN_OK;
}

// ComputeDirection::compute_direction on its own (pnorm_descent.rs:31-36, coordinate_descent.rs:25-45): g goes up, the direction kernel runs, d comes
// down -- the kernels' unit-test entry.  The solver's own g and d are not touched.
static int steep_compute_direction(qn_solver* s, const double* g_host, double* d_host) {
    qn_context* c = s->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = s->n, np = s->T.n_pad;
    if (s->method == QN_PNORM_DESCENT && !s->pnorm_set) return fail(QN_ERROR_INPUT_PARAMS, "inverse_p has not been set (qn_solver_set_inverse_p)");
    if (s->method == QN_PNORM_DESCENT && n <= QN_SMALL_N) { // the reference's literal order, as qn_minimize computes it for these sizes
        std::vector<double> P(n * n), y(n);
        QNCHK(qn_solver_get_inverse_p(s, P.data())); // column-major
        for (size_t i = 0; i < n; ++i) y[i] = P[i] * g_host[0];
        for (size_t j = 1; j < n; ++j)
            for (size_t i = 0; i < n; ++i) { const double t = P[i + j * n] * g_host[j]; y[i] = t + y[i]; }
        for (size_t i = 0; i < n; ++i) d_host[i] = -y[i];
        return QN_OK;
    }
    QNCHK(steep_alloc(s));
    DevBuf<double> buf; // [g | d]
    QNCHK(buf.alloc_zero(2 * np, c->stream));
    HIPCHK(hipMemcpyAsync(buf, g_host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (s->method == QN_PNORM_DESCENT) {
        QNCHK(pnorm_launch(s, buf, buf + np));
        HIPCHK(hipMemcpyAsync(d_host, buf + np, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        s->stats.path |= QN_PATH_PNORM;
        return QN_OK;
    }
    QNCHK(cd_launch(s, buf));
    const int G = s->steep_nshare;
    std::vector<double> part((size_t)3 * G);
    HIPCHK(hipMemcpyAsync(part.data(), s->steep_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double m = 0.0;
    size_t pos = 0;
    for (int b = 0; b < G; ++b) // stage two as the control kernel has it: index order, strict >
        if (part[b] > m) { m = part[b]; pos = (size_t)part[(size_t)G + b]; }
    for (size_t i = 0; i < n; ++i) d_host[i] = 0.0;
    d_host[pos] = -1.0; // -max_value.signum() of a magnitude (coordinate_descent.rs:43)
    return QN_OK;
}
