/*
 * qn_hip.h -- C ABI of libqn_hip.so: the MI355X (gfx950) quasi-Newton / line-search inner loop.
 *
 * This is the drop-in boundary for the hot path of fedemagnani/optimization-solvers
 * (src/ls_solver.rs, src/quasi_newton/{bfgs,dfp}.rs, src/line_search/{mod,backtracking,morethuente}.rs).
 * The reference has no FFI on this path -- its "operator API" is the Rust trait surface -- so every entry
 * point below names the reference item it replaces (file:line relative to the reference repo).  A Rust
 * shim implementing `ComputeDirection` / `LineSearchSolver` on top of these is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; all host matrices are dense f64; `*_host` pointers are host
 * memory, `*_dev` device memory of the context's GPU.  Every function returns a qn_status unless stated;
 * on QN_ABNORMAL_TERMINATION / QN_ERROR_INPUT_PARAMS qn_last_error_message() explains.  There is no CPU
 * fallback: without a usable GPU qn_context_create fails.  All calls on one context must come from one
 * thread at a time (the reference is `&mut self` everywhere: ls_solver.rs:23-112); host callbacks run on
 * the calling thread.
 */
#ifndef QN_HIP_H
#define QN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QN_ABI_VERSION 5

/* SolverError (ls_solver.rs:10-20); 0 is Ok(()) */
typedef enum {
    QN_OK = 0,
    QN_MAX_ITER_REACHED = 1,     /* "Max iter reached"          ls_solver.rs:12-13,110 */
    QN_OUT_OF_DOMAIN = 2,        /* "Out of domain"             ls_solver.rs:14-15,37-40 */
    QN_ERROR_INPUT_PARAMS = 3,   /* "Error in input parameters" ls_solver.rs:16-17 */
    QN_ABNORMAL_TERMINATION = 4  /* "Abnormal termination"      ls_solver.rs:18-19 (HIP / RCCL failures map here) */
} qn_status;

const char* qn_status_string(int status); /* the Display strings of ls_solver.rs:12-19 */
const char* qn_last_error_message(void);  /* thread-local detail of the last non-OK return */
int qn_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Context: one GPU, one HIP stream, optionally one rank of a row-sharded group.
 * The reference has no device or process boundary; this is new.
 * ------------------------------------------------------------------------------------------- */
typedef struct qn_context qn_context;

int qn_device_count(int* out);
int qn_context_create(int device, qn_context** out);

/* Row-sharded group: rank p of `world` owns rows [p*rpr, (p+1)*rpr) of H and of the objective's matrix;
 * all n-vectors are replicated; mat-vec slices are exchanged with one RCCL all-gather per pass.
 * `unique_id` is the 128-byte ncclUniqueId produced by qn_comm_unique_id on rank 0 and distributed by the
 * caller (torch.distributed / MPI / a file). */
#define QN_UNIQUE_ID_BYTES 128
int qn_comm_unique_id(void* out_128_bytes);
int qn_context_create_sharded(int device, int rank, int world, const void* unique_id, qn_context** out);

/* Test / bring-up alternative to RCCL: the caller performs the exchange on host buffers (e.g. with
 * torch.distributed gloo).  `fn(user, sendbuf, recvbuf, count)`: recvbuf[r*count .. (r+1)*count) must
 * receive rank r's sendbuf (an all-gather of `count` doubles per rank).  Returns 0 on success. */
typedef int (*qn_host_allgather_fn)(void* user, const double* sendbuf, double* recvbuf, size_t count);
int qn_context_create_sharded_host_exchange(int device, int rank, int world, qn_host_allgather_fn fn, void* user,
                                            qn_context** out);
/* Row-sharded runs on symmetric storage exchange per-rank PARTIAL n-vectors.  Default (on = 0): one all-gather, every rank adds
 * the P contributions in rank order -- bitwise identical on all ranks, and identical between RCCL and the host-staged exchange.
 * on != 0: ncclAllReduce(ncclSum) instead (the operation north_star names; 1/P of the bytes, RCCL's summation order). */
int qn_context_set_allreduce(qn_context* ctx, int on);
/* Host-exchange contexts only: on != 0 makes every exchange a stream-ordered triple (device-to-pinned copy, the callback as a
 * host node of the stream, pinned-to-device copy) with no synchronisation, so the pipelined launch logic -- which RCCL runs use
 * -- can be rehearsed with several ranks on one GPU.  The callback then runs on a runtime thread, not on the caller's. */
int qn_context_set_host_exchange_async(qn_context* ctx, int on);
/* Row-sharded second-generation runs on a quadratic objective (ABI 5, round 6; DESIGN.md 9.1's fallback): on != 0 lets every evaluation's
 * collective carry the rank's partial n-vector of the TRIAL point beside its 8 KB of scalars (one grouped all-gather), so that an accepted
 * evaluation needs no exchange of its own: E + 1 collectives per iteration instead of E + 2, n doubles per rank more per trial.  For nodes
 * where a small collective between two launches costs much more than its bytes (bench.py --gpus N prints the probed latencies).  The same
 * iterates, bit for bit.  Not together with qn_context_set_allreduce (QN_ERROR_INPUT_PARAMS). */
int qn_context_set_trial_vector_exchange(qn_context* ctx, int on);
void qn_context_destroy(qn_context* ctx);
/* the row partition used for H and the objective's matrix: rows per rank (a multiple of 16) and padded dimension */
int qn_partition(size_t n, int world, size_t* rows_per_rank, size_t* n_pad);
/* diagnostics: create a 1-rank RCCL communicator on this context's GPU, all-gather a small buffer in place on the
 * context's stream and verify it (checks that librccl loads and that the calling convention matches) */
int qn_comm_selftest(qn_context* ctx);
/* collective (every rank calls it): one rank-tagged all-gather through the context's own exchange, then three of different
 * sizes as ONE group (the form the row kernels' exchanges take), each verified on every rank */
int qn_context_comm_check(qn_context* ctx);
/* The latency of ONE exchange (all-gather) of `count` doubles per rank on this context's exchange, between other work on its stream: `reps` timed
 * repetitions bracketed by HIP events; out_us[0] = median, [1] = minimum, [2] = maximum, in microseconds (zeros on a one-rank context).  Collective:
 * call on every rank with the same arguments.  (No counterpart in the reference, which is one thread: bench.py --gpus N reports these in front
 * of its timed region, for the three sizes a row-sharded BFGS iteration exchanges -- 8 KB of scalars, n and 2 n doubles.) */
int qn_context_exchange_probe(qn_context* ctx, size_t count, int reps, double* out_us);
/* measurement aid: the fixed part (ms) of what a hipEventRecord / launch / hipEventRecord bracket on the idle context stream
 * reports beyond the bracketed kernel's own duration: 2 * bracket(one empty kernel) - bracket(two empty kernels) */
int qn_context_event_bracket_overhead(qn_context* ctx, int reps, double* out_ms);
int qn_context_synchronize(qn_context* ctx);
int qn_context_rank(const qn_context* ctx);
int qn_context_world(const qn_context* ctx);
void* qn_context_stream(qn_context* ctx); /* hipStream_t */

/* ---------------------------------------------------------------------------------------------
 * Line searches.  Plain structs by value, as the reference's are plain data.
 *   QN_LS_MORETHUENTE : MoreThuente        (morethuente.rs:6-62, compute_step_len :165-297)
 *   QN_LS_BACKTRACKING: BackTracking       (backtracking.rs:3-58)
 *   QN_LS_NO_SEARCH   : NoSearch           (nosearch.rs:3-15): compute_step_len returns 1.0 and makes no oracle call -- how the reference writes a pure
 *                       Newton step.  Built for the four solvers whose update hook is the trait's default x += t d: QN_GRADIENT_DESCENT, QN_NEWTON,
 *                       QN_COORDINATE_DESCENT, QN_PNORM_DESCENT (and qn_compute_step_len).  NOT BUILT for the quasi-Newton methods, QN_BROYDEN and the
 *                       first-order / projected-Newton family: qn_minimize returns QN_ERROR_INPUT_PARAMS there.
 * ------------------------------------------------------------------------------------------- */
enum { QN_LS_MORETHUENTE = 0, QN_LS_BACKTRACKING = 1,
       QN_LS_MORETHUENTE_B = 2 /* MoreThuenteB, morethuente_b.rs */, QN_LS_BACKTRACKING_B = 3 /* BackTrackingB, backtracking_b.rs */,
       QN_LS_GLL_QUADRATIC = 4 /* GLLQuadratic, gll_quadratic.rs: the non-monotone search of Grippo, Lampariello, Lucidi; QN_SPG / QN_PROJECTED_GRADIENT only */,
       QN_LS_NO_SEARCH = 5 /* NoSearch, nosearch.rs: constant step 1.0 */,
       QN_LS_STRONG_WOLFE = 6 /* StrongWolfe: MINPACK-2 dcsrch; the first-order family, the projected Newton pair, QN_LBFGS and QN_NONLINEAR_CG only */,
       QN_LS_EXACT_QUADRATIC = 7 /* ExactQuadratic: the exact step -g.d / d'Qd on a device quadratic; QN_SPG, QN_PROJECTED_GRADIENT, QN_LBFGS, QN_NONLINEAR_CG only */ };
typedef struct {
    int32_t kind;
    int32_t _pad;
    double c1, c2, t_min, t_max, delta_min, delta, delta_max; /* More-Thuente fields, morethuente.rs:6-14 */
    double bt_c1, bt_beta;                                    /* BackTracking{c1, beta}, backtracking.rs:3-6 */
    /* the *_B variants hold their own box (morethuente_b.rs:14-15, backtracking_b.rs:7-8): host vectors of length n,
     * read by qn_minimize; NULL = unbounded side */
    const double* lower_bound_host;
    const double* upper_bound_host;
} qn_linesearch;
/* GLLQuadratic (gll_quadratic.rs:3-10) travels in the fields above, the struct keeps its layout: kind = QN_LS_GLL_QUADRATIC, c1 = c1,
 * _pad = m (the look-back, :6), delta_min = sigma1, delta_max = sigma2.  m = 0 or m > 64 makes qn_minimize return QN_ERROR_INPUT_PARAMS: the
 * history f_previous (:7) is a fixed ring of 64 values on the device.  ONE DIFFERENCE FROM THE REFERENCE: this struct is plain data passed
 * by value, so the history belongs to the SOLVER, not to the line-search value -- it survives successive qn_minimize calls on one solver
 * (as the reference's survives successive minimize calls with one GLLQuadratic), and qn_solver_reset empties it. */

void qn_morethuente_default(qn_linesearch* ls);                      /* MoreThuente::default, morethuente.rs:16-28 */
int qn_morethuente_with_deltas(qn_linesearch* ls, double dmin, double d, double dmax); /* :31-41 */
int qn_morethuente_with_t_min(qn_linesearch* ls, double t_min);      /* :42-45 */
int qn_morethuente_with_t_max(qn_linesearch* ls, double t_max);      /* :46-49 */
int qn_morethuente_with_c1(qn_linesearch* ls, double c1);            /* :50-55; the assert!s become QN_ERROR_INPUT_PARAMS */
int qn_morethuente_with_c2(qn_linesearch* ls, double c2);            /* :56-62 */
void qn_backtracking_new(qn_linesearch* ls, double c1, double beta); /* BackTracking::new, backtracking.rs:8-10 */
void qn_morethuente_b_new(qn_linesearch* ls);                          /* MoreThuenteB::new(n): defaults, bounds -inf/+inf, morethuente_b.rs:18-31 */
void qn_backtracking_b_new(qn_linesearch* ls, double c1, double beta, const double* lower_bound_host, const double* upper_bound_host); /* backtracking_b.rs:10-23 */
void qn_linesearch_with_lower_bound(qn_linesearch* ls, const double* lower_bound_host); /* morethuente_b.rs:32-35 */
void qn_linesearch_with_upper_bound(qn_linesearch* ls, const double* upper_bound_host); /* morethuente_b.rs:36-39 */
void qn_nosearch_new(qn_linesearch* ls);                               /* NoSearch, nosearch.rs:3 */
void qn_gll_quadratic_new(qn_linesearch* ls, double c1, size_t m);                      /* GLLQuadratic::new, gll_quadratic.rs:13-23: sigma1 = 0.1, sigma2 = 0.9 */
void qn_gll_quadratic_with_sigmas(qn_linesearch* ls, double sigma1, double sigma2);     /* :24-28 */
/* StrongWolfe (QN_LS_STRONG_WOLFE; no counterpart among the reference's line searches): the strong-Wolfe search as published -- MINPACK-2 `dcsrch` / `dcstep`
 * (More' and Thuente, ACM TOMS 20, 1994; the search the Fortran L-BFGS-B runs) -- for QN_SPG, QN_PROJECTED_GRADIENT, QN_PROJECTED_NEWTON,
 * QN_SPECTRAL_PROJECTED_NEWTON, QN_LBFGS and QN_NONLINEAR_CG; every other method: QN_ERROR_INPUT_PARAMS.  ONE oracle call per trial: the bracket keeps (f, f') of its
 * end points (the reference's More-Thuente transcription evaluates two or three points per inner iteration, morethuente.rs:181-294).  It travels in
 * the fields above: kind = QN_LS_STRONG_WOLFE, c1 = ftol (1e-4), c2 = gtol (0.9), delta = xtol (0.1), t_min = stpmin (0), t_max = stpmax (1e10);
 * qn_morethuente_with_t_min / _with_t_max set the last two.  qn_minimize checks 0 < c1 < c2 < 1, xtol >= 0 and 0 <= t_min <= t_max
 * (QN_ERROR_INPUT_PARAMS).  The first trial is min(max(1, stpmin), stpmax).  The search ends on the strong-Wolfe conditions, on stp = stpmax with
 * sufficient decrease and a derivative <= c1 g.d, on stp = stpmin, on the xtol test and on the rounding-error test; the returned step is then the one
 * just evaluated.  When max_iter_line_search runs out the next step is returned unevaluated, as by this family's other searches.
 * A trial whose f (or directional derivative) is NOT FINITE counts as "sufficient decrease fails, derivative positive": the bracket shrinks onto
 * [best step, this step] and the next trial bisects it (dcsrch has no rule for that case).
 * g.d >= 0 at the start of a search (dcsrch's input error) ends qn_minimize with QN_ABNORMAL_TERMINATION, "not a descent direction", x at x_k:
 * ProjectedLBFGS with an active box can meet it (d = P(x - H g) - x need not descend).
 * BOXED FORM: once qn_linesearch_with_lower_bound / _with_upper_bound gave it a box of its own (as the *_B searches hold one), every search runs
 * with stpmax = min(t_max, min_i ratio_i), the ratio of morethuente_b.rs:185-197.  The clip is recomputed per search and NOT written back into
 * t_max (the struct is not modified).  trace: ls_cases holds dcstep's case (1 .. 4; 5: a non-finite trial; 0: returned) per trial, base 8, and
 * bit 30 when the search switched to its second stage.  qn_compute_step_len: QN_ERROR_INPUT_PARAMS for this kind. */
void qn_strong_wolfe_new(qn_linesearch* ls, double c1, double c2);
int qn_strong_wolfe_with_xtol(qn_linesearch* ls, double xtol);
/* ExactQuadratic (QN_LS_EXACT_QUADRATIC; no counterpart among the reference's line searches): on f = 1/2 x'Qx - b'x the minimiser along d is
 * t = -g.d / d'Qd.  It costs ONE product q = Q d (the curvature pass of qn_objective_hess_vec), after which g(x + t d) = g + t q and
 * f(x + t d) = f + t (g.d + (t / 2) d'Qd) need no second pass over the matrix.  No value of f is ever compared: the step is accepted as it is.  With
 * QN_NONLINEAR_CG this is linear conjugate gradients.
 * Methods: QN_SPG, QN_PROJECTED_GRADIENT, QN_LBFGS (free and with a box), QN_NONLINEAR_CG; objectives: the dense and the sparse device quadratic.
 * QN_ERROR_INPUT_PARAMS with the reason in qn_last_error_message: a host closure, a device closure or log-sum-exp ("the exact step needs a device
 * quadratic"), every other method, qn_compute_step_len, a search with a box of its own (lower_bound_host / upper_bound_host set), refresh_every < 0.
 * ONE SEARCH: (1) the loop top leaves g.d; unless g.d < 0 the run ends with QN_ABNORMAL_TERMINATION ("ExactQuadratic: not a descent direction"),
 * x at x_k; (2) q = Q d and c = d.q (products and sums round separately, fixed orders); (3) unless c > 0 and finite: QN_ABNORMAL_TERMINATION
 * ("ExactQuadratic: non-positive curvature along the direction"), x at x_k; (4) t = (-g.d) / c, one division; on a solver with a box t = min(t, 1)
 * (a comparison): there d = P(x - z) - x, so t <= 1 keeps x + t d feasible; (5) xt = x + t d, t d rounded first; (6) (f_t, gt) at xt: on a REFRESH
 * iteration the objective's own launches, otherwise gt_i = g_i + t q_i (t q_i rounded first) and f_t = f + t (g.d + (0.5 t) c); (7) accepted.
 * REFRESH: refresh_every = r travels in `_pad`.  r = 1 (what every binding's default is): the objective evaluates every accepted point -- two matrix
 * passes per iteration, every gradient a true one.  r = k > 1: every k-th accepted point (the count survives calls, qn_solver_reset clears it).
 * r = 0: never -- except that the first evaluation at x is always the objective's, and that CONVERGENCE IS DECLARED ONLY ON A TRUE GRADIENT: when the
 * loop top's test passes on a gradient that came from the recurrence, the run does not stop; x is evaluated by the objective (a forced refresh,
 * counted) and the loop top runs again.  The oracle's `memoize` is not consulted: the evaluation of the accepted point is always kept.
 * qn_stats: oracle_evals counts evaluations by the objective only; curvature passes are reported by qn_solver_exact_state and counted in obj_bytes
 * (sparse: 12 nnz + 4 (n + 1) + 16 n each; dense: the matrix once) and in launches. */
void qn_exact_quadratic_new(qn_linesearch* ls, int refresh_every);

/* ---------------------------------------------------------------------------------------------
 * Oracle: `impl FnMut(&DVector<f64>) -> FuncEvalMultivariate` (ls_solver.rs:69, func_eval.rs:4-41).
 * ------------------------------------------------------------------------------------------- */
/* host closure: writes *f and g[0..n); return value 0 (the reference closure cannot fail; non-zero aborts
 * the run with QN_ABNORMAL_TERMINATION). */
typedef int (*qn_host_oracle_fn)(void* user, const double* x_host, size_t n, double* f, double* g_host);
/* device closure: enqueue work on `stream` that reads x_dev[0..n) and writes *f_dev and g_dev[0..n). */
typedef int (*qn_device_oracle_fn)(void* user, void* stream, const double* x_dev, size_t n, double* f_dev, double* g_dev);
/* Newton only: the Hessian part of the FuncEval (func_eval.rs:8,27-33) at x, column-major n x n (like DMatrix).  QN_NEWTON takes its
 * Hessian from this closure, from a device quadratic (its own matrix: one step) or from a device log-sum-exp objective (formed on the
 * device at every x_k, once per iteration at the loop top whatever `memoize` says: qn_objective_hessian); a device closure has none. */
typedef int (*qn_host_hessian_fn)(void* user, const double* x_host, size_t n, double* h_colmajor_host);

typedef struct qn_objective qn_objective; /* a device-resident objective owned by the library */

enum { QN_ORACLE_HOST = 0, QN_ORACLE_DEVICE_FN = 1, QN_ORACLE_OBJECTIVE = 2 };
typedef struct {
    int32_t kind;
    /* 0: reproduce the reference's call sequence exactly (loop-top call ls_solver.rs:79, every line-search
     *    call incl. the per-iteration re-evaluation at tl morethuente.rs:217, and bfgs.rs:98);
     * 1: evaluate each DISTINCT point once (the oracle must then be a pure function of x).  The values fed
     *    to the algorithm are identical; only the number of evaluations changes (5 -> 2 per iteration for
     *    More-Thuente on a quadratic). */
    int32_t memoize;
    qn_host_oracle_fn host_fn;
    void* host_user;
    qn_device_oracle_fn device_fn;
    void* device_user;
    qn_objective* objective;
    qn_host_hessian_fn host_hessian_fn; /* Newton with a host closure; device objectives (quadratic, log-sum-exp) supply their own Hessian */
} qn_oracle;

/* Built-in benchmark objective (build-defined): f = 1/2 x'Qx - b'x, g = Qx - b.
 * `q_rowmajor_host` is the full symmetric n x n matrix; each rank uploads only its own rows.  (A matrix that is not symmetric
 * bit for bit is multiplied as given -- the symmetric-storage evaluation is then not used.) */
int qn_quadratic_create(qn_context* ctx, size_t n, const double* q_rowmajor_host, const double* b_host, qn_objective** out);
/* Same objective with Q generated on the device, shard-locally: off-diagonal Q_ij = u(seed,min,max)/n,
 * u in [-1,1) from a counter-based splitmix64 hash; diagonal given (SPD if diag_i >= 1). */
int qn_quadratic_create_synthetic(qn_context* ctx, size_t n, uint64_t seed, const double* diag_host, const double* b_host,
                                  qn_objective** out);
/* f = log sum_i exp(a_i'x + c_i) + mu/2 ||x||^2; A is m x n row-major, rows sharded. */
int qn_logsumexp_create(qn_context* ctx, size_t m, size_t n, const double* a_rowmajor_host, const double* c_host, double mu,
                        qn_objective** out);
/* Regularised logistic regression: f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2, g = -A'(y o w o s) + mu x with s_i = 1 / (1 + exp(y_i a_i'x)),
 * H = A' diag(d) A + mu I with d_i = w_i s_i (1 - s_i).  A is m x n row-major and dense; y_i is EXACTLY -1 or +1 (0 / 1 labels: pass 2 y - 1; any other
 * value: QN_ERROR_INPUT_PARAMS -- a 0 never masks a row silently); w_host holds m sample weights >= 0, finite (a negative or non-finite one:
 * QN_ERROR_INPUT_PARAMS), NULL: all ones.  A row with w_i = 0 is masked: it adds nothing to f, g or H, the value is that of the problem with the row
 * deleted.  mu: any finite value.  n_pad <= 16384 and one rank (otherwise QN_ERROR_INPUT_PARAMS, "not built").  One evaluation is TWO launches
 * (csrc/qn_logistic.hip.h): one stream of A, 8 m n_pad bytes, stable for every finite margin; no atomics, the same bits for the same x from run to run
 * and from object to object.  It runs under QN_SPG, QN_PROJECTED_GRADIENT, QN_LBFGS, QN_NONLINEAR_CG and QN_NEWTON_CG with every line search those take
 * but ExactQuadratic; every other method: QN_ERROR_INPUT_PARAMS.  qn_objective_hess_vec_at gives H(x) v (one weights pass of A at x, one product pass);
 * qn_objective_hess_vec, qn_objective_hessian and qn_objective_sparse_info on it: QN_ERROR_INPUT_PARAMS; qn_objective_get_rows returns rows of A. */
int qn_logistic_create(qn_context* ctx, size_t m, size_t n, const double* a_rowmajor_host, const double* y_host, const double* w_host, double mu,
                       qn_objective** out);
/* The same objective with a SPARSE A: m x n in CSR (the columns of a row strictly increasing), with NO limit on n_pad -- logistic regression at the
 * sizes the O(n) solvers are for.  Labels, weights, masking and mu follow qn_logistic_create's rules exactly.  The two index arrays travel as
 * untyped pointers: `index_bytes` = 4 (int32) or 8 (int64) holds for BOTH; on the device they are int32.  At creation the host also builds the CSR
 * of A' (a counting sort) and BOTH copies go to the device: 24 bytes per nonzero.  The transpose product g = A'coef walks the rows of A' with the
 * kernel that walks the rows of A, so it uses no float atomic and every sum has one fixed order: the same bits for the same x from run to run and
 * from object to object.  Each copy has its own static cut over workgroups, its own long rows (more than 2048 entries: a whole workgroup each --
 * a dense column of A, such as an intercept column, is a long row of A') and its own lanes per row.  Validated on the host in O(nnz), each failure
 * QN_ERROR_INPUT_PARAMS: a null pointer, m == 0 or n == 0, index_bytes not 4 or 8, m or n > 2^30, nnz > 2^31 - 1, row_ptr[0] != 0,
 * row_ptr[m] != nnz, a decreasing row_ptr, a column outside [0, n), unsorted or duplicate columns, a bad label or weight, a non-finite mu, a
 * row-sharded context ("single-GPU").  A failed creation leaks nothing and leaves *out alone.  One evaluation is THREE launches
 * (csrc/qn_sparse_logistic.hip.h): the row pass (margins, coefficients, d, the loss), the column pass (g, ||x||^2) and a one-workgroup finish.
 * It runs under QN_SPG, QN_PROJECTED_GRADIENT, QN_LBFGS, QN_NONLINEAR_CG and QN_NEWTON_CG with every line search those take but ExactQuadratic;
 * every other method, qn_objective_hessian, qn_objective_hess_vec, qn_objective_get_rows and qn_objective_sparse_info: QN_ERROR_INPUT_PARAMS.
 * qn_objective_eval works on it; qn_objective_hess_vec_at gives H(x) v = A'(d o (A v)) + mu v (a weights pass at x, the product's two passes, a fold). */
int qn_sparse_logistic_create(qn_context* ctx, size_t m, size_t n, size_t nnz, const void* row_ptr_host, const void* col_idx_host, int index_bytes,
                              const double* values_host, const double* y_host, const double* w_host, double mu, qn_objective** out);
/* Lanes that share one row in the row pass (over A) and in the column pass (over A'): each 1, 2, 4, 8, 16, 32 or 64, or 0 for the choice made at
 * creation from that copy's mean row length.  Another value may change the bits of f, g and H v; the results stay inside the same error bounds. */
int qn_sparse_logistic_set_lanes(qn_objective* objective, int lanes_rows, int lanes_cols);
/* nnz, the lanes per row in use for each pass, and the long rows of A and of A' (any pointer may be NULL).  Another objective: QN_ERROR_INPUT_PARAMS. */
int qn_sparse_logistic_info(qn_objective* objective, size_t* nnz, int* lanes_rows, int* lanes_cols, size_t* n_long_rows, size_t* n_long_cols);
/* Regularised softmax (multinomial logistic) regression on a dense A (m x n row-major): labels y_i in {0, .., K-1} (labels_i32_host: m int32 values),
 * sample weights w_i >= 0 (w_host, NULL: all ones; a weight of 0 masks its row: it adds nothing to f, g or H), K = n_classes >= 2, any finite mu.
 * The parameter vector is CLASS-MAJOR: x[k n + j] = W[k, j], N = K n entries with no padding between classes (sklearn's coef_ raveled); g and H v use
 * the same layout, and the objective's dimension -- what a solver is created with -- is N.
 *     f = sum_i w_i (logsumexp_k a_i.W_k - a_i.W_{y_i}) + mu/2 ||x||^2,   g_k = sum_i w_i (p_ik - [y_i = k]) a_i + mu W_k,   p_i = softmax_k(a_i.W_k)
 *     (H v)_k = sum_i w_i p_ik (u_ik - sum_l p_il u_il) a_i + mu V_k,   u_ik = a_i.V_k
 * A label outside [0, K), a negative or non-finite weight, a non-finite mu: QN_ERROR_INPUT_PARAMS, with the index.  A class that no row carries is
 * legal.  Not built (QN_ERROR_INPUT_PARAMS before anything is allocated): a row-sharded context, a padded K n above 16384 (W stays on chip), K < 2,
 * K > 256; every shape inside these limits runs.  One evaluation is TWO launches (csrc/qn_multinomial.hip.h): ONE stream of A serves all K classes, stable for every finite margin; no
 * atomics, the same bits for the same x from run to run and from object to object.  It runs under QN_SPG, QN_PROJECTED_GRADIENT, QN_LBFGS,
 * QN_NONLINEAR_CG and QN_NEWTON_CG with every line search those take but ExactQuadratic; every other method: QN_ERROR_INPUT_PARAMS.
 * qn_objective_hess_vec_at gives H(x) v (one weights pass of A at x, one product pass); qn_objective_hess_vec, qn_objective_hessian,
 * qn_objective_get_rows and qn_objective_sparse_info on it: QN_ERROR_INPUT_PARAMS. */
int qn_multinomial_create(qn_context* ctx, size_t m, size_t n, size_t n_classes, const double* a_rowmajor_host, const void* labels_i32_host,
                          const double* w_host, double mu, qn_objective** out);
/* The class probabilities at x (N entries, class-major): p_host receives m x K row-major, P[i, k] = p_ik; a masked row's are stored as zeros (they are
 * the Hessian's weights).  One weights pass of A. */
int qn_multinomial_probabilities(qn_objective* objective, const double* x_host, double* p_host);
/* Which kernel streams A: 1 the register-blocked kernel on the vector unit (every shape inside the limits), 2 the v_mfma_f64_16x16x4_f64 kernel (K <= 64
 * where its cut and its LDS fit; otherwise QN_ERROR_INPUT_PARAMS and nothing changes), 0 the automatic choice, which a new objective has.  The two
 * kernels sum in different orders: each gives the same bits from run to run, not the other's. */
int qn_multinomial_set_kernel(qn_objective* objective, int kernel);
/* The same softmax regression on a SPARSE A (m x n in CSR, the columns of a row strictly increasing; the index arrays as qn_sparse_logistic_create
 * takes them): qn_multinomial_create's function, labels, weights, mu and CLASS-MAJOR parameter vector x[k n + j] = W[k, j] of N = K n entries, with
 * no limit on K n and none on K.  The device holds A AND A' (24 bytes per nonzero) and feature-major copies of x and of A'C with the padded leading
 * dimension Kp (qn_sparse_multinomial_info); no float atomic, every sum in one fixed order: the same bits for the same x from run to run, from
 * object to object and for int32 and int64 indices.  Each failure QN_ERROR_INPUT_PARAMS before anything is allocated: a null pointer, m == 0 or
 * n == 0, index_bytes not 4 or 8, K < 2, m or n > 2^30, nnz > 2^31 - 1, m K > 2^31 - 1, K n > 2^30, a bad CSR pattern (qn_sparse_logistic_create's
 * rules), a label outside [0, K) or a negative or non-finite weight (with the index), a non-finite mu, a row-sharded context ("single-GPU").  A
 * failed creation leaks nothing and leaves *out alone.  One evaluation is FIVE launches (csrc/qn_sparse_multinomial.hip.h): x to feature-major, the
 * row pass (margins, softmax, C, P, the loss), the column pass (A'C), back to class-major (+ mu x, ||x||^2) and a one-workgroup finish.  It runs
 * under QN_SPG, QN_PROJECTED_GRADIENT, QN_LBFGS, QN_NONLINEAR_CG and QN_NEWTON_CG with every line search those take but ExactQuadratic; every other
 * method, qn_objective_hessian, qn_objective_hess_vec, qn_objective_get_rows, qn_objective_sparse_info and the qn_multinomial_* / qn_sparse_logistic_*
 * calls: QN_ERROR_INPUT_PARAMS.  qn_objective_eval works on it; qn_objective_hess_vec_at gives H(x) v (a weights pass at x, the product's five launches). */
int qn_sparse_multinomial_create(qn_context* ctx, size_t m, size_t n, size_t n_classes, size_t nnz, const void* row_ptr_host, const void* col_idx_host,
                                 int index_bytes, const double* values_host, const void* labels_i32_host, const double* w_host, double mu,
                                 qn_objective** out);
/* nnz, the entry lanes per row in use for each pass, the long rows of A and of A', and Kp (any pointer may be NULL).  Another objective:
 * QN_ERROR_INPUT_PARAMS. */
int qn_sparse_multinomial_info(qn_objective* objective, size_t* nnz, int* lanes_rows, int* lanes_cols, size_t* n_long_rows, size_t* n_long_cols, int* kp);
/* Entry lanes L that share one row in the row pass (over A) and in the column pass (over A'): each 1, 2, 4, 8, 16, 32 or 64, or 0 for the choice made
 * at creation; min(64 / L, the next power of two of K) class lanes stand beside each.  Another value may change the bits of f, g and H v; the
 * results stay inside the same error bounds. */
int qn_sparse_multinomial_set_lanes(qn_objective* objective, int lanes_rows, int lanes_cols);
/* The class probabilities at x (N entries, class-major): p_host receives m x K row-major; a masked row's are zeros.  One weights pass. */
int qn_sparse_multinomial_probabilities(qn_objective* objective, const double* x_host, double* p_host);
/* f = 1/2 x'Qx - b'x, g = Qx - b with a SPARSE Q: n x n in CSR, both triangles of a symmetric matrix -- the device objective that exists at the
 * sizes the O(n) solvers are for.  It runs under QN_SPG, QN_PROJECTED_GRADIENT and QN_LBFGS with every line search those take; every other method:
 * QN_ERROR_INPUT_PARAMS ("unsupported objective"; the projected Newton pair: "Hessian not available in the oracle").  One rank (a row-sharded
 * context: QN_ERROR_INPUT_PARAMS).  The two index arrays travel as untyped pointers: `index_bytes` = 4 (int32) or 8 (int64) holds for BOTH, as in
 * scipy's CSR; on the device they are int32, 12 bytes per nonzero.  Validated on the host in O(nnz), each failure QN_ERROR_INPUT_PARAMS: a null
 * pointer or n == 0, index_bytes not 4 or 8, n > 2^30, nnz > 2^31 - 1, row_ptr[0] != 0, row_ptr[n] != nnz, a decreasing row_ptr, a column outside
 * [0, n), columns not STRICTLY increasing inside a row (unsorted or duplicate).  nnz == 0 is legal (g = -b).  A matrix that is not symmetric bit
 * for bit (pattern and values; qn_objective_sparse_info reports it) is multiplied as given, as qn_quadratic_create's is.  One evaluation is two
 * launches (csrc/qn_sparse.hip.h): CSR-vector with `lanes_per_row` lanes to a row and whole workgroups for rows of more than 2048 entries, f's
 * shares added in a fixed order -- no atomics, the same bits for the same x from run to run and from object to object.
 * qn_objective_get_rows / qn_objective_hessian on it: QN_ERROR_INPUT_PARAMS. */
int qn_sparse_quadratic_create(qn_context* ctx, size_t n, size_t nnz, const void* row_ptr_host, const void* col_idx_host,
                               int index_bytes, const double* values_host, const double* b_host, qn_objective** out);
/* lanes that share one row: 1, 2, 4, 8, 16, 32 or 64; 0: chosen from the mean row length (the default).  Another value may change the bits of f and g
 * (another summation order), never between two evaluations with the same value. */
int qn_sparse_quadratic_set_lanes_per_row(qn_objective* obj, int lanes);
/* a sparse quadratic's shape: its nonzeros, the lanes per row in use, the rows summed by a workgroup of their own, whether Q == Q' bit for bit.
 * Any pointer may be NULL.  Another objective: QN_ERROR_INPUT_PARAMS. */
int qn_objective_sparse_info(qn_objective* obj, size_t* nnz, int* lanes_per_row, size_t* n_long_rows, int* symmetric);
void qn_objective_destroy(qn_objective* obj);
/* one evaluation at a host point (tests, and `let eval = f_and_g(x)` after minimize as in examples/quadratic.rs:39) */
int qn_objective_eval(qn_objective* obj, const double* x_host, double* f, double* g_host);
/* download rows [row0,row0+nrows) of this rank's matrix shard (row-major, n columns); rows outside the shard fail */
int qn_objective_get_rows(qn_objective* obj, size_t row0, size_t nrows, double* out_host);
/* the Hessian at a host point, column-major n x n like DMatrix: the `hessian()` part of a FuncEval (func_eval.rs:8,27-33) for a binding to
 * attach after qn_minimize.  A quadratic returns Q (x is not read).  A log-sum-exp objective returns
 * A' (diag(p) - p p') A + mu I, p = softmax(A x + c), formed on the device by the kernel QN_NEWTON runs (csrc/qn_lse_hess.hip.h): symmetric
 * bit for bit, the same bits for the same x.  The n_pad x n_pad device matrix is allocated by the first call.  h_colmajor_host == NULL: the
 * launches run and are waited for, nothing is downloaded.  One rank (a row-sharded context: QN_ERROR_INPUT_PARAMS). */
int qn_objective_hessian(qn_objective* obj, const double* x_host, double* h_colmajor_host);
/* the Hessian-vector product of a quadratic at a host vector: q = Q v into q_host (n entries; NULL: not downloaded) and the curvature v'Qv into
 * *vqv -- what the exact step t = -g.d / d'Qd along d costs, and what a binding needs for a conjugate-gradient loop of its own.  One pass over
 * the matrix and no evaluation of f.  A sparse quadratic: the CSR kernel's curvature form (csrc/qn_sparse.hip.h) -- the structure, the lanes per
 * row and the summation order inside a row of an evaluation, so q has the bits an evaluation at v with b = 0 gives g; 12 nnz + 4 (n + 1) + 16 n
 * bytes, 8 n fewer than an evaluation.  A dense quadratic: the row kernel of an evaluation with the point set to v, then one workgroup that forms
 * v.q.  v'Qv's products and sums round separately, in a fixed order: the same bits for the same v from run to run and from object to object.
 * Log-sum-exp: QN_ERROR_INPUT_PARAMS (not built: its Hessian depends on a point, see qn_objective_hess_vec_at).  One rank (a row-sharded
 * context: QN_ERROR_INPUT_PARAMS). */
int qn_objective_hess_vec(qn_objective* obj, const double* v_host, double* q_host, double* vqv);
/* the Hessian-vector product AT A POINT: q = H(x) v into q_host (n entries; NULL: not downloaded) and v'H(x)v into *vhv, without the matrix.
 * Log-sum-exp: H v = A'(p o (A v)) - gbar (p . (A v)) + mu v with p = softmax(A x + c), gbar = A'p -- the weights at x (two passes of A, the launches
 * qn_objective_hessian starts with), then ONE stream of A (8 m n bytes, what an evaluation moves; csrc/qn_lse_hv.hip.h) where the dense Hessian costs
 * O(m n^2) flops and 8 n^2 bytes.  Rows with p_k = 0 (c_k = -inf) add nothing.  Fixed summation orders, no atomics: the same bits for the same
 * (x, v) from run to run and from object to object.  Built where the one-pass evaluation exists, n_pad <= 16384, and on one rank; otherwise
 * QN_ERROR_INPUT_PARAMS ("not built").  A dense or a sparse quadratic: x is not read (it may be NULL) and the call IS qn_objective_hess_vec -- the
 * same launches, the same bits.  (qn_objective_hess_vec itself still answers "not built" on log-sum-exp: it has no point to form p at.) */
int qn_objective_hess_vec_at(qn_objective* obj, const double* x_host, const double* v_host, double* q_host, double* vhv);
/* the DIAGONAL of the Hessian at a point: diag_host[j] = H(x)_jj for j < n, without the matrix -- what a Jacobi preconditioner divides by, and a
 * scaling a binding may want for its own conjugate-gradient loop.  The weights at x (the kind's weights pass), then one pass over A with squared
 * entries.  Logistic: M_j = sum_i d_i a_ij^2 + mu; log-sum-exp: M_j = sum_i p_i a_ij^2 - gbar_j^2 + mu (ONE stream of the dense A, 8 m n bytes, and a
 * combine launch: csrc/qn_hess_diag.hip.h); sparse logistic: M_j = sum_{i in column j} d_i a_ij^2 + mu in one launch over the device's copy of A'
 * (an empty column gives mu).  Rows with a zero weight add nothing.  Fixed summation orders, no atomics: the same bits for the same x from run to
 * run, from object to object, and for int32 / int64 indices.  The dense kinds: built where the product is (n_pad <= 16384, one rank).  A multinomial
 * or a sparse multinomial objective and the two quadratics: QN_ERROR_INPUT_PARAMS before anything is launched (not built). */
int qn_objective_hess_diag_at(qn_objective* obj, const double* x_host, double* diag_host);

/* ---------------------------------------------------------------------------------------------
 * Solvers: BFGS (bfgs.rs:4-127), DFP (dfp.rs), Broyden (broyden.rs), GradientDescent (gradient_descent.rs:7-82), Newton (newton/mod.rs).
 * ------------------------------------------------------------------------------------------- */
enum { QN_BFGS = 0, QN_DFP = 1, QN_GRADIENT_DESCENT = 2, QN_NEWTON = 3 /* newton/mod.rs:8-69, SURVEY.md 8(f) row f2 */,
       QN_SR1 = 4 /* sr1_b.rs (row f4; SR1B once qn_solver_set_bounds is called) */,
       /* The first-order family: O(n) state (no inverse Hessian), one rank, every vector operation on a device-wide grid (QN_PATH_VECTOR).
        * Line searches: QN_LS_GLL_QUADRATIC, QN_LS_BACKTRACKING, QN_LS_BACKTRACKING_B, QN_LS_STRONG_WOLFE (More-Thuente: QN_ERROR_INPUT_PARAMS).  The box is
        * qn_solver_set_bounds' (-inf, +inf without it).  trace: gnorm = ||projected gradient||_inf (ls_solver.rs:121-133), s_norm = ||s|| (SPG).
        * qn_solver_reset projects x0 onto the box, as ::new does (spg.rs:35).  qn_solver_compute_direction on these methods is a HOST utility for
        * bindings (it downloads x and the box and forms P(x - lambda g) - x in a host loop); qn_minimize forms its directions on the device.
        * Device closures and device objectives are enqueued a whole iteration at a time, ahead of the device-side decisions: the LAST batch of a
        * run that ends at its loop top (convergence or an out-of-domain f) still evaluates once at a stale point.  That evaluation is not used
        * and not counted in qn_stats; a device closure that counts its own invocations sees one more than oracle_evals reports for such a run
        * (none for a run that ends on the iteration cap, none for SPG's constructor evaluation).  Host closures are called only for points the solver asked for. */
       QN_SPG = 5 /* SpectralProjectedGradient, steepest_descent/spg.rs */,
       QN_PROJECTED_GRADIENT = 6 /* ProjectedGradientDescent, steepest_descent/projected_gradient_descent.rs */,
       /* The second-order box-constrained pair (newton/projected_newton.rs, newton/spn.rs): the first-order family's machine, line searches (QN_LS_STRONG_WOLFE among them), box,
        * trace, callbacks and warm restarts, with z = H^-1 g where that family has g: d = P(x - z) - x, and d = P(x - lambda z) - x with SPG's
        * lambda (qn_solver_set_spg_lambdas / qn_solver_spg_lambda answer for QN_SPECTRAL_PROJECTED_NEWTON too).  z is `hessian.cholesky().unwrap()
        * .solve(g)`: one blocked Cholesky (Newton's, on the f64 matrix cores) and one pair of triangular solves per iteration; ONLY THE LOWER
        * TRIANGLE of the Hessian is read.  The Hessian is a host closure's host_hessian_fn or a device quadratic's own matrix; a device closure or
        * a log-sum-exp objective has none here: QN_ERROR_INPUT_PARAMS ("Hessian not available in the oracle").  A Hessian whose Cholesky fails
        * ends qn_minimize with QN_ABNORMAL_TERMINATION and x at x_k (the reference panics on the unwrap; there is no LU fallback).
        * QN_PROJECTED_NEWTON keeps s_norm / y_norm (qn_solver_s_norm, qn_solver_y_norm, the two *_too_close getters) and tests them at the loop
        * top in the reference's order: s_norm, y_norm, then the projected gradient (projected_newton.rs:95-110); trace: s_norm, y_norm.
        * One n x n work matrix, allocated by the first qn_minimize that computes a direction.  One rank. */
       QN_PROJECTED_NEWTON = 7 /* ProjectedNewton, newton/projected_newton.rs */,
       QN_SPECTRAL_PROJECTED_NEWTON = 8 /* SpectralProjectedNewton, newton/spn.rs */,
       /* Broyden (quasi_newton/broyden.rs; BroydenB, broyden_b.rs, once qn_solver_set_bounds is called): BFGS's skeleton -- d = -H g (P(x - H g) - x
        * when bounded), s_norm / y_norm tests and skip rule, the oracle call sequence -- with the update H += ((s - H y) s') H / (s . y) AS WRITTEN
        * (broyden.rs:115-118): rank-1, H + c a w' with a = s - H y, w = H' s, c = 1 / s.y.  H is NOT symmetric after the first update, and the secant
        * equation does not hold.  Line searches: every one but QN_LS_GLL_QUADRATIC.  Every oracle kind; one rank (a row-sharded context:
        * QN_ERROR_INPUT_PARAMS); synchronous requests; the full row-major H streamed once per iteration by csrc/qn_rank1.hip.h (QN_PATH_RANK1).
        * qn_solver_set_inv_hessian accepts any matrix. */
       QN_BROYDEN = 9 /* Broyden, quasi_newton/broyden.rs */,
       /* The two remaining members of the steepest-descent family.  Both run beside QN_GRADIENT_DESCENT on the control-step machine: the default hook
        * x += t d, has_converged = ||g||_inf < grad_tol with the NaN-ignoring max, no s_norm / y_norm, no evaluation at the accepted point; every line
        * search QN_GRADIENT_DESCENT takes, and QN_LS_NO_SEARCH; every oracle kind; memoize 0 / 1; callbacks, trace, warm restarts.  One rank (a
        * row-sharded context: QN_ERROR_INPUT_PARAMS); synchronous requests.
        * QN_COORDINATE_DESCENT (coordinate_descent.rs:30-44, AS WRITTEN): p = the FIRST index of the largest |g_i| (strict >, a NaN never wins; no
        * positive magnitude at all: p = 0) and d = -max_value.signum() e_p.  max_value is a MAGNITUDE, so its signum is +1.0: d = -e_p WHATEVER THE SIGN
        * OF g_p.  On a coordinate with a negative gradient that is an ascent direction, and BackTracking returns beta^max_iter_line_search.  Reference
        * behaviour, reproduced.  On the device: a two-stage (magnitude, index) reduction (cd_argmax_kernel, then the control kernel).
        * QN_PNORM_DESCENT (pnorm_descent.rs:35): d = (-inverse_p) * g with the caller's dense matrix (qn_solver_set_inverse_p; qn_minimize without
        * one: QN_ERROR_INPUT_PARAMS).  ONE read-only stream of the matrix per iteration -- 8 n^2 bytes, csrc/qn_pnorm.hip.h (QN_PATH_PNORM) -- whose launch
        * also leaves g.d and ||g||_inf; n <= 5: the reference's literal column sweep.  h_passes / h_bytes of qn_stats count those streams. */
       QN_COORDINATE_DESCENT = 10 /* CoordinateDescent, steepest_descent/coordinate_descent.rs */,
       QN_PNORM_DESCENT = 11 /* PnormDescent, steepest_descent/pnorm_descent.rs */,
       /* Limited-memory BFGS (ProjectedLBFGS once qn_solver_set_bounds is called): the quasi-Newton method whose state is O(m n) and not O(n^2) -- the last
        * m pairs (s, y), m = 5 by default as Lbfgsb::new (quasi_newton/lbfgsb.rs:91), 1 <= m <= QN_LBFGS_MAX_M (qn_solver_set_lbfgs_memory).  It runs on the
        * first-order family's machine (QN_PATH_VECTOR | QN_PATH_LBFGS) and takes that family's line searches (QN_LS_GLL_QUADRATIC, QN_LS_BACKTRACKING,
        * QN_LS_BACKTRACKING_B, and QN_LS_STRONG_WOLFE -- the search that keeps s.y > 0 on a free problem, so that every pair is committed;
        * More-Thuente: QN_ERROR_INPUT_PARAMS), box, loop top (||projected gradient||_inf < tol; no s_norm / y_norm tests), trace
        * (gnorm = that norm, s_norm = ||s||, updated = the pair was committed), callbacks and warm restarts (the memory survives calls; qn_solver_reset
        * empties it); every oracle kind, memoize 0 / 1, one rank.  The direction is d = P(x - z) - x with z = H_k g from the COMPACT FORM of Byrd, Nocedal
        * and Schnabel (1994): two streams of the memory and one small solve per iteration (csrc/qn_lbfgs.hip.h), gamma = s_k.y_k / y_k.y_k
        * (QN_OPT_LBFGS_UNIT_SCALING: gamma = 1).  A pair is kept only when s.y > DBL_EPSILON y.y; when g.z <= 0 or is not finite the memory is cleared
        * and z = g (counted: qn_solver_lbfgs_state).  Profiling mode times this method's three direction launches apart: t_hpass_ms = the Gram kernel, t_hreduce_ms = the
        * apply kernel, t_ereduce_ms = vec_dir_kernel on z.  y needs the gradient at the accepted point: the oracle is called there as for QN_SPG.
        * THIS IS NOT THE REFERENCE'S `Lbfgsb` (an optional binding to the Fortran L-BFGS-B library): there is no generalised Cauchy point and no
        * subspace minimisation.  The bounded variant follows this library's own BFGSB convention, d = P(x - H g) - x (bfgs_b.rs:72-75); with an active
        * box that direction is no more guaranteed to descend than BFGSB's is.  qn_solver_compute_direction: QN_ERROR_INPUT_PARAMS (use qn_minimize). */
       QN_LBFGS = 12 /* limited-memory BFGS; no counterpart in the reference's default feature set */,
       /* Nonlinear conjugate gradient: the O(n) method whose state is ONE extra vector -- the direction last searched -- where L-BFGS(m) keeps 2 (m + 1).
        * d+ = beta d - g+ (beta d rounds first, then the difference); beta by the variant of qn_solver_set_cg (QN_CG_PR_PLUS after qn_solver_create),
        * with y = g+ - g: FR g+.g+ / g.g; PR+ max(0, g+.y / g.g); HS+ max(0, g+.y / d.y); DY g+.g+ / d.y; HZ (Hager and Zhang 2005) max(betaN, eta_k),
        * betaN = (g+.y - 2 (y.y)(g+.d) / d.y) / d.y, eta_k = -1 / (||d|| min(0.01, ||g||)).  The rules, in this order: (1) the first direction after
        * qn_solver_create / qn_solver_reset / qn_solver_set_cg is -g (not a restart); (2) restart_every > 0 and that many iterations since the last -g
        * direction: beta = 0; (3) the formula, plain IEEE divisions; (4) beta not finite: 0; (5) Powell's test, |g+.g| >= powell_nu g+.g+ : 0 (0.2 by
        * default, +inf: off); (6) unless -g+.g+ + beta (g+.d) < 0 -- descent, from the sums alone -- 0.  Every beta that ends as exactly 0 counts as a
        * restart (qn_solver_cg_state); the trace's `updated` is beta != 0, s_norm = ||s||, gnorm = ||g||_inf.  It runs on the first-order family's
        * machine (QN_PATH_VECTOR | QN_PATH_CG, csrc/qn_cg.hip.h): the accept pass leaves every inner product beta needs, so the direction costs one
        * stream (16 n bytes read, 16 n written) and no reduction launch of its own.  UNBOUNDED ONLY: qn_solver_set_bounds gives QN_ERROR_INPUT_PARAMS,
        * as does qn_solver_compute_direction (use qn_minimize).  Line searches: QN_LS_STRONG_WOLFE (what FR, DY and HS+ assume), QN_LS_BACKTRACKING and,
        * on a device quadratic, QN_LS_EXACT_QUADRATIC (the exact step: linear conjugate gradients);
        * QN_LS_GLL_QUADRATIC, QN_LS_BACKTRACKING_B and both More-Thuente kinds: QN_ERROR_INPUT_PARAMS.  Every oracle kind of the family, memoize 0 / 1,
        * trace, callbacks, warm restarts (the direction and beta survive calls: two calls of k iterations give the bits of one call of 2 k), one rank.
        * The first trial step of every search is 1, as everywhere in this family.  Profiling mode: t_hpass_ms = cg_dir_kernel, t_hreduce_ms =
        * cg_accept_kernel.  Not built: a box, preconditioning, an initial-step rule, qn_compute_step_len. */
       QN_NONLINEAR_CG = 13 /* nonlinear conjugate gradient; no counterpart in the reference */,
       /* Truncated Newton: Newton's direction from a few conjugate-gradient steps on H z = g, each costing ONE Hessian-vector product and never a
        * matrix -- the method between dense Newton (O(m n^2) flops and 8 n^2 bytes per iteration) and the O(n) solvers that keep no curvature.  The
        * objectives are the device log-sum-exp (qn_logsumexp_create) and the device logistic regression (qn_logistic_create: H = A' diag(d) A +
        * mu I, the same kernels with a zero gbar, ONE pass of A for the weights d at x_k), n_pad <= 16384, one rank; the product is one stream of A
        * (csrc/qn_lse_hv.hip.h, qn_objective_hess_vec_at).  The sparse logistic regression (qn_sparse_logistic_create) has no limit on n_pad: its
        * product is a row pass over A, a column pass over A' and a one-workgroup fold (csrc/qn_sparse_logistic.hip.h).  A closure or a quadratic: QN_ERROR_INPUT_PARAMS (on a quadratic the method is linear
        * conjugate gradients, which QN_NONLINEAR_CG with QN_LS_EXACT_QUADRATIC already is).  UNBOUNDED ONLY (qn_solver_set_bounds:
        * QN_ERROR_INPUT_PARAMS).  Line searches: QN_LS_BACKTRACKING and QN_LS_STRONG_WOLFE without a box of its own, first trial t = 1 (the Newton
        * direction is scaled); every other search: QN_ERROR_INPUT_PARAMS.  It runs on the first-order family's machine (QN_PATH_VECTOR |
        * QN_PATH_NEWTON_CG, csrc/qn_newton_cg.hip.h): memoize 0 / 1, trace (gnorm = ||g||_inf), callbacks and warm restarts as for QN_LBFGS; the
        * convergence test is the machine's, ||g||_inf < tol at the loop top.  THE RULES of one direction, in this order:
        *   1. p = softmax(A x_k + c), gbar = A'p: two passes of A (the loop top's one-pass evaluation keeps no normalised p);
        *   2. z = 0, r = g, p = g, gg = g.g, rr = gg, j = 0, eta = min(eta_max, sqrt(sqrt(gg)));
        *   3. q = H p = A'(p o (A p)) - gbar (p . (A p)) + mu p, kappa = p.q;
        *   4. unless kappa > 0 and finite: neg_curv += 1; if j == 0 then z = g; the loop ends;
        *   5. alpha = rr / kappa; z += alpha p, r -= alpha q (alpha p and alpha q round first, no FMA); j += 1; rr' = r.r;
        *   6. sqrt(rr') <= eta sqrt(gg): the loop ends (tolerance); else j == max_inner: it ends (cap);
        *   7. beta = rr' / rr; p = r + beta p (beta p rounds first); rr = rr'; back to 3;
        *   8. behind the loop: g.z > 0 and finite, or else z = g and fallbacks += 1 (QN_LBFGS's safeguard; after rule 4 at j = 0 z is g and the
        *      test is not made); d = -z, written directly (not through P(x - z) - x).
        * Inner products: product and sum round separately, fixed orders, no atomics: the same bits from run to run.  The host enqueues the inner
        * steps `chunk` at a time with the rest of the iteration behind them, all predicated on the device's control block, and reads that block
        * once per batch: host_syncs <= sum_k max(1, ceil(j_k / chunk)) + extra trials + 2; the chunk never changes a bit.  qn_stats: obj_bytes
        * counts 8 m n_pad per product and 16 m n_pad per weights pass; profiling mode: t_newton_ms = the product launches, t_hpass_ms = the
        * method's O(n) streams.  Not built: n_pad > 16384, a box, preconditioning, a trust region, row sharding, qn_compute_step_len,
        * qn_solver_compute_direction (QN_ERROR_INPUT_PARAMS). */
       QN_NEWTON_CG = 14 /* truncated Newton (Newton-CG) on the log-sum-exp Hessian-vector product; no counterpart in the reference */,
       /* Spectral proximal gradient (SpaRSA: Wright, Nowak, Figueiredo 2009): min f(x) + sum_j l1_j |x_j| over lb <= x <= ub, l1_j >= 0 finite, one scalar
        * or one value per entry (qn_solver_set_l1; 0 after qn_solver_create).  QN_SPG with the projection replaced by the proximal map of lambda l1 |.| plus
        * the box, on the same machine (QN_PATH_VECTOR | QN_PATH_PROX, csrc/qn_vec_prox.hip.h): every oracle kind of the family, memoize 0 / 1, box, trace,
        * callbacks, one peek per batch, warm restarts (lambda, the ring and the memo survive calls: two calls of k iterations give the bits of one call of
        * 2 k); qn_solver_set_spg_lambdas / qn_solver_spg_lambda answer for it, and the first qn_minimize makes the constructor's call for lambda0 =
        * clamp(1 / ||d||_inf) with lambda = 1.  THE RULES, per entry, each operation rounded once, no FMA:
        *   1. sg = lambda g_j; u = x_j - sg; tau = lambda l1_j; z = u - tau if u > tau, u + tau if u < -tau, else 0.0; p = fmin(fmax(z, lb_j), ub_j);
        *      d_j = p - x_j.  Where the prox returns 0, d_j = -x_j and an accepted unit step leaves x_j = 0.0 exactly.
        *   2. the convergence measure replaces the projected gradient: the element of least magnitude of [lo, hi], lo = hi = g_j + l1_j (x_j > 0),
        *      g_j - l1_j (x_j < 0), lo = g_j - l1_j and hi = g_j + l1_j (x_j == 0); lo = -inf where x_j == lb_j, hi = +inf where x_j == ub_j; QN_OK when the
        *      largest magnitude is < tol.  It is the trace's gnorm.
        *   3. h0 = h(x), h1 = sum_j l1_j |x_j + d_j|, Delta = g.d + (h1 - h0), F_k = f + h0 (the trace's f).  Out-of-domain is tested on f; the sign of
        *      Delta is not tested.
        *   4. the search along d, first trial t = 1, F_t = f(x + t d) + h(x + t d): QN_LS_GLL_QUADRATIC (the ring holds composite values) and
        *      QN_LS_BACKTRACKING, with F_t, F_k, Delta where SPG has f_t, f_k, g.d.  Every other search, qn_compute_step_len and
        *      qn_solver_compute_direction: QN_ERROR_INPUT_PARAMS before any launch.
        *   5. accept and lambda = clamp(s.s / s.y), lambda_max when s.y <= 0: QN_SPG's.
        * With l1 == 0 everywhere the run is QN_SPG's, bit for bit.  One rank.  Not built: backtracking on lambda, acceleration, group penalties. */
       QN_SPECTRAL_PROXIMAL_GRADIENT = 15 /* SpectralProximalGradient: L1-regularised SPG by soft-thresholding; no counterpart in the reference */,
       /* Orthant-wise limited-memory quasi-Newton (OWL-QN: Andrew and Gao, ICML 2007): min f(x) + sum_j l1_j |x_j|, unbounded, l1 as for
        * QN_SPECTRAL_PROXIMAL_GRADIENT (qn_solver_set_l1).  QN_LBFGS's memory, compact-form direction and commit rule on the same machine
        * (QN_PATH_VECTOR | QN_PATH_LBFGS | QN_PATH_OWLQN, csrc/qn_vec_owlqn.hip.h), with four element-wise steps of its own.  Every oracle kind of
        * QN_LBFGS, memoize 0 / 1, trace, callbacks, one peek per batch, warm restarts (two calls of k iterations give the bits of one call of 2 k);
        * qn_solver_set_lbfgs_memory, qn_solver_lbfgs_state and QN_OPT_LBFGS_UNIT_SCALING answer for it.  THE RULES, each operation rounded once, no FMA:
        *   1. the pseudo-gradient v_j = g_j + l1_j (x_j > 0), g_j - l1_j (x_j < 0); at x_j == 0: g_j - l1_j if that is > 0, g_j + l1_j if that is < 0,
        *      else 0.  QN_OK when ||v||_inf < tol (QN_SPECTRAL_PROXIMAL_GRADIENT's measure without a box); it is the trace's gnorm.  Out-of-domain is
        *      tested on the smooth f.
        *   2. z = H_k v by QN_LBFGS's kernels (the safeguard reads v.z > 0 and leaves z = v; no pair: z = v).
        *   3. d_j = -z_j where l1_j == 0 or z_j and v_j have the same strict sign, else 0.0.  v.d not < 0 or not finite: QN_ABNORMAL_TERMINATION, "not a
        *      descent direction", x left at x_k.
        *   4. the orthant xi_j = sign(x_j), or sign(-v_j) where x_j == 0.
        *   5. the trial xt_j = x_j + t d_j (t d_j rounded first) where l1_j == 0 or that value has xi_j's strict sign, else 0.0; first trial t = 1.
        *   6. QN_LS_BACKTRACKING only, accepted when F_t - F_k <= c1 v.(xt - x) (no factor t), F = f + h; a non-finite F_t shrinks without counting.  Every
        *      other search, a box, qn_compute_step_len and qn_solver_compute_direction: QN_ERROR_INPUT_PARAMS before any launch.
        *   7. x_next = xt (never x + t d); s = x_next - x, y the difference of the SMOOTH gradients; the pair is kept when s.y > DBL_EPSILON y.y.
        *   8. trace: f = F_k, gnorm = ||v||_inf, updated = the pair was kept.
        *   9. the memory, gamma, the resets and the memo survive calls; qn_solver_set_l1 keeps the pairs, x and the memo; qn_solver_set_lbfgs_memory drops
        *      the pairs.
        * One rank.  Not built: a box, StrongWolfe or a non-monotone search, an initial step 1 / ||v||, group penalties. */
       QN_OWLQN = 16 /* OWLQN: orthant-wise L-BFGS for L1-regularised objectives; no counterpart in the reference */ };
#define QN_LBFGS_MAX_M 32
/* QN_NONLINEAR_CG's variants (qn_solver_set_cg) */
enum { QN_CG_FR = 0 /* Fletcher-Reeves */, QN_CG_PR_PLUS = 1 /* Polak-Ribiere+ */, QN_CG_HS_PLUS = 2 /* Hestenes-Stiefel+ */, QN_CG_DY = 3 /* Dai-Yuan */,
       QN_CG_HZ = 4 /* Hager-Zhang */ };
typedef struct qn_solver qn_solver;

/* BFGS::new(tol, x0) / DFP::new / GradientDescent::new(grad_tol, x0): H = I (no identity copy is kept) */
int qn_solver_create(qn_context* ctx, int method, double tol, const double* x0_host, size_t n, qn_solver** out);
void qn_solver_destroy(qn_solver* s);
/* Row f4: BFGSB / DFPB / SR1B / BroydenB (bfgs_b.rs:43-77, dfp_b.rs, sr1_b.rs, broyden_b.rs): box bounds on a BFGS / DFP / SR1 / Broyden solver.  The current x
 * is projected (bfgs_b.rs:49) and every direction becomes P(x - H g) - x (bfgs_b.rs:72-75). */
int qn_solver_set_bounds(qn_solver* s, const double* lower_bound_host, const double* upper_bound_host);
/* QN_SPG: with_lambdas (spg.rs:23-27; defaults 1e-3 / 1e3, :36-37; the current lambda is not clamped again).  Other methods: QN_ERROR_INPUT_PARAMS. */
int qn_solver_set_spg_lambdas(qn_solver* s, double lambda_min, double lambda_max);
/* QN_SPG: lambda(), the Barzilai-Borwein scalar.  SpectralProjectedGradient::new calls the oracle (spg.rs:40-46); qn_solver_create has none, so
 * the first qn_minimize after create / reset makes that call (counted in oracle_calls; with memoize = 1 the point is evaluated once):
 * is_some = 0 until then.  A qn_minimize with max_iter_solver = 0 does just that and returns QN_MAX_ITER_REACHED. */
int qn_solver_spg_lambda(qn_solver* s, double* out, int* is_some);
/* QN_SPECTRAL_PROXIMAL_GRADIENT: the penalty h(x) = sum_j l1_j |x_j| -- l1_host's n entries, or l1_scalar for every entry when l1_host is NULL.  A
 * negative or non-finite value, or another method: QN_ERROR_INPUT_PARAMS.  Between two qn_minimize calls it clears GLLQuadratic's ring (its values
 * belong to the old penalty) and keeps lambda, x and the memoised evaluation of the smooth part: the regularisation-path use. */
int qn_solver_set_l1(qn_solver* s, const double* l1_host, double l1_scalar);
/* ... and the n entries in use (a scalar: n copies). */
int qn_solver_get_l1(qn_solver* s, double* l1_host);
/* (QN_OWLQN takes both as well; there qn_solver_set_l1 leaves the memory of pairs as it is: they are differences of the smooth gradient.)
 * QN_OWLQN: the pseudo-gradient v of the last loop top (rule 1), n entries; zeros before the first one.  Other methods: QN_ERROR_INPUT_PARAMS. */
int qn_solver_get_pseudo_gradient(qn_solver* s, double* out_host);
/* QN_PROJECTED_NEWTON / QN_SPECTRAL_PROJECTED_NEWTON: Cholesky factorisations enqueued by the last qn_minimize.  With a device quadratic the factor
 * is kept between iterations and calls (keyed on the objective; QN_OPT_PNEWTON_REUSE_FACTOR): 1 for the first call, 0 afterwards; with a host
 * closure, or with the option off, one per iteration that computed a direction.  Other methods: 0.
 * (The count comes back through a size_t*, like every other count in this header, and not through a uint64_t*: the ABI check that compares this
 * header with the Python and Rust mirrors knows the pointer types the header already used.  Both are 64 bits wide on every platform ROCm runs on.) */
int qn_solver_newton_factorisations(qn_solver* s, size_t* out);
/* QN_LBFGS: the memory m (pairs kept at most; 5 after qn_solver_create).  Outside 1 .. QN_LBFGS_MAX_M, or on another method: QN_ERROR_INPUT_PARAMS.
 * The stored pairs are dropped.  The vectors -- 2 (m + 1) n_pad doubles -- are allocated by the next qn_minimize. */
int qn_solver_set_lbfgs_memory(qn_solver* s, size_t m);
/* QN_LBFGS: m, the pairs stored now, the scaling gamma of the last direction (1 before the first pair), and how often the safeguard g.z > 0 has
 * cleared the memory since qn_solver_create / qn_solver_reset.  Any pointer may be NULL.  Other methods: QN_ERROR_INPUT_PARAMS. */
int qn_solver_lbfgs_state(qn_solver* s, size_t* m, size_t* stored, double* gamma, size_t* resets);
/* QN_NONLINEAR_CG: the variant (QN_CG_*; QN_CG_PR_PLUS after qn_solver_create), Powell's nu (0.2; +inf disables the test; NaN or <= 0:
 * QN_ERROR_INPUT_PARAMS) and restart_every (0: never).  An unknown variant, or another method: QN_ERROR_INPUT_PARAMS.  The stored direction is
 * dropped: the next direction is -g. */
int qn_solver_set_cg(qn_solver* s, int variant, double powell_nu, size_t restart_every);
/* QN_NONLINEAR_CG: the variant, the beta of the last accepted iteration (0 before the first), the betas that ended as exactly 0 and the iterations
 * since the last -g direction, since qn_solver_create / qn_solver_reset.  Any pointer may be NULL.  Other methods: QN_ERROR_INPUT_PARAMS. */
int qn_solver_cg_state(qn_solver* s, int* variant, double* beta, size_t* restarts, size_t* since_restart);
/* QN_NEWTON_CG: the forcing term's cap eta_max (0.5 after qn_solver_create; outside (0, 1): QN_ERROR_INPUT_PARAMS), the inner steps of one
 * direction at the most (0, the default: min(n, 100)) and the inner steps enqueued per batch (8; 0: QN_ERROR_INPUT_PARAMS).  Another method:
 * QN_ERROR_INPUT_PARAMS. */
int qn_solver_set_newton_cg(qn_solver* s, double eta_max, size_t max_inner, size_t chunk);
/* QN_NEWTON_CG, of the last qn_minimize: the inner steps of the last direction, of all directions, the Hessian-vector products (one per inner
 * step started), the times rule 4 met curvature that was not positive, and the times rule 8 replaced z by g.  Any pointer may be NULL.
 * Another method: QN_ERROR_INPUT_PARAMS. */
int qn_solver_newton_cg_state(qn_solver* s, size_t* inner_last, size_t* inner_total, size_t* hv_passes, size_t* neg_curv, size_t* fallbacks);
/* NewtonCG's preconditioner for the inner conjugate-gradient loop.  QN_PRECOND_NONE (the default): plain CG, nothing changes.  QN_PRECOND_JACOBI: the
 * diagonal of H(x_k), by the objective's own diagonal pass (qn_objective_hess_diag_at's launches) once per outer iteration behind the weights -- one
 * more stream of A, about the price of one inner step.  minv_j = 1 / M_j where M_j > 0 and finite, else 1; p = minv o r + beta p with alpha = rz / kappa,
 * beta = rz' / rz, rz = r.(minv o r); the loop still ends on the EUCLIDEAN residual, sqrt(r.r) <= eta sqrt(g.g), so eta means the same with and
 * without it.  It pays where the columns of A differ in scale by orders of magnitude (2 to 4 times fewer inner steps); it buys nothing on
 * well-scaled columns, where the extra pass is pure cost, and it can lose with m < n and a small mu.  QN_ERROR_INPUT_PARAMS: another method, another
 * value; at qn_minimize, an objective without a Hessian diagonal (a multinomial pair, before anything is launched).  The setting survives calls and
 * qn_solver_reset. */
enum { QN_PRECOND_NONE = 0, QN_PRECOND_JACOBI = 1 };
int qn_solver_set_newton_cg_preconditioner(qn_solver* s, int kind);
/* the setting, and of the last qn_minimize: the directions that started with a diagonal pass, and how many entries of the LAST minv rule 2' set to 1
 * (M_j not positive or not finite).  Any pointer may be NULL. */
int qn_solver_newton_cg_precond_state(qn_solver* s, int* kind, size_t* diag_passes, size_t* floored_last);
/* what the last diagonal pass of a preconditioned run left: M = diag H(x) into m_host and 1 / M by the rule above into minv_host, n entries each
 * (either may be NULL).  x is the point of the run's last loop top: the last direction's, or the final point of a run that ended there.  QN_ERROR_INPUT_PARAMS: another method, or no run with QN_PRECOND_JACOBI has been made. */
int qn_solver_newton_cg_precond_diag(qn_solver* s, double* m_host, double* minv_host);
/* QN_LS_EXACT_QUADRATIC, of the last qn_minimize: the curvature passes, the accepted points (and forced re-evaluations of x) that the objective
 * evaluated -- the first evaluation at x is not counted --, and the last search's step and curvature d'Qd.  Any pointer may be NULL.  A solver
 * outside the first-order family: QN_ERROR_INPUT_PARAMS. */
int qn_solver_exact_state(qn_solver* s, size_t* curvature_passes, size_t* refreshes, double* last_t, double* last_curvature);
/* QN_PNORM_DESCENT: inverse_p of PnormDescent::new(grad_tol, x0, inverse_p) (pnorm_descent.rs:20-27) and its getter; column-major n x n, like DMatrix
 * and like qn_solver_set_inv_hessian.  ANY matrix is accepted: the reference tests neither symmetry nor definiteness.  It is a constructor argument,
 * not state: qn_solver_reset keeps it.  Other methods: QN_ERROR_INPUT_PARAMS. */
int qn_solver_set_inverse_p(qn_solver* s, const double* p_colmajor_host);
int qn_solver_get_inverse_p(qn_solver* s, double* out_colmajor_host);
/* back to the state right after BFGS::new(tol, x0): x = x0, H = I, k = 0, s_norm = y_norm = None */
int qn_solver_reset(qn_solver* s, const double* x0_host);

/* callback: Option<&mut dyn FnMut(&Self)> (ls_solver.rs:72,105-107); called after k += 1 */
typedef void (*qn_callback_fn)(void* user, qn_solver* solver);

/* LineSearchSolver::minimize (ls_solver.rs:66-111).  Resets k only (warm restart keeps x, H, s_norm, y_norm). */
/* `ls` is not const: MoreThuenteB clips its t_max to the box and keeps it clipped (morethuente_b.rs:201 `self.t_max = ...`). */
int qn_minimize(qn_solver* s, qn_linesearch* ls, const qn_oracle* oracle, size_t max_iter_solver,
                size_t max_iter_line_search, qn_callback_fn callback, void* callback_user);

/* LineSearch::compute_step_len (line_search/mod.rs:14-23) on its own, as the reference's line-search tests call it
 * (backtracking.rs:65-113, morethuente.rs:303-352, morethuente_b.rs:330-385): step length along `direction` from `x_k`, where
 * (f_k, g_k) is the evaluation at x_k.  Runs the device state machine from the line search's first statement to its return;
 * `ls` is updated as by qn_minimize (MoreThuenteB keeps its clipped t_max). */
int qn_compute_step_len(qn_context* ctx, qn_linesearch* ls, const double* x_k_host, double f_k, const double* g_k_host,
                        const double* direction_host, size_t n, const qn_oracle* oracle, size_t max_iter, double* step_out);

/* getters generated by derive_getters on bfgs.rs:3-12, plus LineSearchSolver::xk/k (bfgs.rs:52-63) */
size_t qn_solver_n(const qn_solver* s);
size_t qn_solver_k(const qn_solver* s);                    /* k() */
int qn_solver_set_k(qn_solver* s, size_t k);               /* k_mut() (bfgs.rs:58-63) */
double qn_solver_tol(const qn_solver* s);                  /* tol() */
int qn_solver_get_x(qn_solver* s, double* out_host);       /* x() / xk() */
int qn_solver_set_x(qn_solver* s, const double* x_host);   /* xk_mut() */
/* The vector family (SPG, projected gradient, projected Newton, L-BFGS, NonlinearCG, NewtonCG), for an audit of a run from its own vectors: n
 * doubles copied from the solver's vectors on its stream; no launch, and a run that never calls them is unchanged bit for bit.
 * get_direction: the direction of the last accepted iteration.  Inside the callback this is d_k of the iteration just reported (the next batch is
 * not enqueued before the callback returns).  QN_ERROR_INPUT_PARAMS when none is held: before the first accepted iteration of a call, and after a
 * call whose last loop top ended it (convergence: that loop top left P(x - g) - x in the vector, which was never searched).
 * get_gradient: the gradient of the evaluation held at the current x.  Inside the callback, on a memoised oracle, this is g_{k+1}, the accepted
 * trial's gradient; after a call that converged it is the gradient that passed the test.  QN_ERROR_INPUT_PARAMS when no evaluation at x is held:
 * nothing evaluated yet (an iteration cap of 0 evaluates nothing, as in the reference), an oracle that is not memoised (the next loop top
 * evaluates x itself), or x set since.  Under ExactQuadratic it is the gradient the run holds, which may be the recurrence's.
 * Another method: QN_ERROR_INPUT_PARAMS. */
int qn_solver_get_direction(qn_solver* s, double* d_host);
int qn_solver_get_gradient(qn_solver* s, double* g_host);
int qn_solver_s_norm(qn_solver* s, double* out, int* is_some); /* s_norm(): Option<f64> */
int qn_solver_y_norm(qn_solver* s, double* out, int* is_some); /* y_norm(): Option<f64> */
int qn_solver_next_iterate_too_close(qn_solver* s, int* out);          /* bfgs.rs:15-20 */
int qn_solver_gradient_next_iterate_too_close(qn_solver* s, int* out); /* bfgs.rs:21-26 */
int qn_solver_decrement_squared(qn_solver* s, double* out, int* is_some); /* Newton: decrement_squared(): Option<f64>, newton/mod.rs:10 */
/* approx_inv_hessian(): column-major n x n.  Lazy: applies the pending rank-2 update and gathers this rank's
 * rows; rows of other ranks are left untouched unless `all_ranks` (then an all-gather fills everything). */
int qn_solver_get_inv_hessian(qn_solver* s, double* out_colmajor_host, int all_ranks);
int qn_solver_set_inv_hessian(qn_solver* s, const double* h_colmajor_host);
/* ComputeDirection::compute_direction on its own (bfgs.rs:42-49, dfp.rs:42-49: -H g; gradient_descent.rs:24-30: -g), for a
 * binding that implements the trait; qn_minimize computes its directions on the device and never calls this. */
int qn_solver_compute_direction(qn_solver* s, const double* g_host, double* d_host);
/* The inverse-Hessian half of the `update_next_iterate` hook on its own (bfgs.rs:92-130, dfp.rs:92-118), again for a binding
 * that implements LineSearchSolver hook by hook: records s_norm / y_norm, skips the update when either is below tol
 * (bfgs.rs:103-109), else applies the BFGS / DFP / Broyden update to the device-resident matrix (Broyden: also when bounded). */
int qn_solver_secant_update(qn_solver* s, const double* s_host, const double* y_host);

/* ---- build-side instrumentation (not in the reference) ---- */
#define QN_TRACE_LS_MODIFIED (1 << 30)
typedef struct {
    double f, gnorm, t, s_norm, y_norm; /* f(x_k), ||g_k|| (inf-norm for gradient descent), step, ||s||, ||y|| */
    int32_t n_evals;   /* oracle calls of the reference's sequence in this iteration (memoised ones included) */
    int32_t ls_iters;  /* line-search inner iterations started */
    int32_t ls_cases;  /* More-Thuente: base-8 digits, one per inner iteration: 1..4 trial case, 0 returned;
                        * bit 30 (QN_TRACE_LS_MODIFIED): the modified-updating switch (morethuente.rs:212-215) was thrown */
    int32_t updated;   /* 1 if the inverse Hessian was updated */
} qn_trace_rec;
/* record up to `cap` iterations of the next qn_minimize calls; x_trace (optional) gets x_{k+1} rows */
int qn_solver_set_trace(qn_solver* s, size_t cap, int with_x);
int qn_solver_get_trace(qn_solver* s, qn_trace_rec* out_host, size_t cap, size_t* len, double* x_trace_host);

typedef struct {
    uint64_t iterations;       /* outer iterations completed by the last qn_minimize */
    uint64_t oracle_calls;     /* calls of the reference's sequence */
    uint64_t oracle_evals;     /* evaluations actually performed (distinct points when memoize = 1) */
    uint64_t h_passes;         /* passes over the inverse Hessian */
    uint64_t h_bytes;          /* algorithmic bytes moved over H by those passes (this rank) */
    uint64_t obj_bytes;        /* algorithmic bytes read from the objective's matrix (this rank) */
    uint64_t launches;         /* kernels enqueued */
    uint64_t host_syncs;       /* stream synchronisations */
    double   t_hpass_ms, t_eval_ms, t_ctl_ms, t_comm_ms; /* HIP-event time per kernel class (profiling mode) */
    uint64_t n_hpass_timed, n_eval_timed, n_ctl_timed, n_comm_timed;
    uint64_t matrix_bytes_per_pass; /* bytes of H (or Q) one pass of the last run streams on this rank: the rank's rows, or -- on the
                                       symmetric-storage path -- the 128 x 128 tiles of the symmetric half this rank owns */
    /* The counters above describe the LAST qn_minimize call (the device control block restarts them with k, ls_solver.rs:74).
     * These accumulate over every qn_minimize call made on this solver, so a harness that makes several calls (warm-up,
     * timed region, restarts after convergence) can difference them. */
    uint64_t total_minimize_calls, total_iterations, total_oracle_calls, total_oracle_evals, total_h_passes, total_h_bytes,
        total_obj_bytes;
    uint32_t path; /* QN_PATH_* flags of the last call: which kernels serviced it */
    uint32_t _pad;
    /* profiling mode, symmetric-storage path: the small second launch of a pass (slot sums + epilogue), timed on its own;
     * t_hpass_ms / t_eval_ms then hold the tile kernels alone */
    double   t_hreduce_ms, t_ereduce_ms;
    uint64_t n_hreduce_timed, n_ereduce_timed;
    /* row-sharded runs: collectives enqueued by every qn_minimize call of this solver so far -- of n-vectors (mat-vec partials:
     * the all-reduce north_star names, as an all-gather + rank-order sum or as ncclAllReduce), and of per-workgroup scalars
     * (8 KB per rank: what an evaluation hands the line search on the second-generation path) */
    uint64_t total_xchg_vector, total_xchg_scalar;
    /* Newton (newton/mod.rs:26-49), profiling mode: HIP-event time of the direction requests (staging, factorisation, the four
     * triangular sweeps of d = -H^-1 g and of the decrement's second solve) */
    double   t_newton_ms;
    uint64_t n_newton_timed;
    /* pivoted-LU path: times a bounded wait of the one-launch panel / sweep kernels expired and the factorisation was run again
     * with one launch per step (a co-tenant on the GPU can do that; the result is the same, the iteration slower) */
    uint64_t newton_lu_sync_timeouts;
    /* second-generation path, last qn_minimize call: steps of the state machine that a kernel's prologue took as the straight-line code of the steady
     * iteration instead of the generic machine (QN_OPT_MACHINE_FAST_STEPS; one in the accept-reduce and one in the update tiles per steady iteration) */
    uint64_t fast_machine_steps;
    /* second-generation path, last qn_minimize call: update passes that applied the pending update in registers and did NOT store the matrix
     * (QN_OPT_HPASS_STORE_SKIP: the pass behind them applies two updates and stores), and the bytes of H the call's passes really read and wrote --
     * h_bytes stays the algorithmic size, every pass counted as one read and one write of the streamed tiles */
    uint64_t n_hpass_nostore;
    uint64_t h_bytes_moved;
} qn_stats;
#define QN_PATH_FUSED 1u       /* fused fast path (device quadratic, memoised): no kernel but the streaming ones touches an n-vector */
#define QN_PATH_SYM 2u         /* ... on the symmetric half of H and Q only */
#define QN_PATH_SYM_GENERIC 4u /* generic path whose H pass runs on the symmetric half */
#define QN_PATH_PIPELINED 8u   /* predicated kernels enqueued ahead of the device-side decisions (no host sync per step) */
#define QN_PATH_SYM2 16u       /* QN_PATH_SYM with the solver's decisions taken in every kernel's prologue (5 launches per iteration) */
#define QN_PATH_TILES1 32u     /* QN_PATH_SYM2 whose update pass streams H through the first-generation tile kernel (one workgroup per tile) behind a
                                  one-workgroup launch that runs the state machine: H's share past the Infinity Cache, and the log-sum-exp objective */
#define QN_PATH_VECTOR 64u     /* the first-order family's device-wide vector kernels (csrc/qn_vec.hip.h): QN_SPG, QN_PROJECTED_GRADIENT */
#define QN_PATH_PNEWTON 128u   /* ... with the direction from a Cholesky solve: QN_PROJECTED_NEWTON, QN_SPECTRAL_PROJECTED_NEWTON (set beside QN_PATH_VECTOR) */
#define QN_PATH_RANK1 256u     /* QN_BROYDEN's H passes: the square-tile kernel of csrc/qn_rank1.hip.h (non-symmetric rank-1 update, row AND column sums in one stream of H) */
#define QN_PATH_PNORM 512u     /* QN_PNORM_DESCENT's directions: pnorm_dir_kernel of csrc/qn_pnorm.hip.h (one read-only stream of inverse_p, with g.d and ||g||_inf in the same launch) */
#define QN_PATH_LBFGS 1024u    /* QN_LBFGS: the direction from the compact form of L-BFGS, two streams of the memory per iteration (csrc/qn_lbfgs.hip.h); set beside QN_PATH_VECTOR */
#define QN_PATH_CG 2048u       /* QN_NONLINEAR_CG: the direction d = beta p - g written by cg_dir_kernel, beta from the accept pass's sums (csrc/qn_cg.hip.h); set beside QN_PATH_VECTOR */
#define QN_PATH_EXACT 4096u    /* QN_LS_EXACT_QUADRATIC: the step from one curvature pass, (f, g) of the accepted point by the recurrence or by the objective (csrc/qn_vec_exact.hip.h); set beside QN_PATH_VECTOR */
#define QN_PATH_PROX 16384u    /* QN_SPECTRAL_PROXIMAL_GRADIENT: the direction from the proximal map of lambda l1 |.| plus the box, the search on composite values (csrc/qn_vec_prox.hip.h); set beside QN_PATH_VECTOR */
#define QN_PATH_OWLQN 32768u   /* QN_OWLQN: the pseudo-gradient, the aligned direction and the orthant projection of the trial point around QN_LBFGS's direction kernels (csrc/qn_vec_owlqn.hip.h); set beside QN_PATH_VECTOR | QN_PATH_LBFGS */
#define QN_PATH_NEWTON_CG 8192u /* QN_NEWTON_CG: the direction from conjugate gradients on H z = g, one log-sum-exp Hessian-vector product per inner step (csrc/qn_newton_cg.hip.h, qn_lse_hv.hip.h); set beside QN_PATH_VECTOR */
int qn_solver_get_stats(qn_solver* s, qn_stats* out);
/* profiling != 0: bracket every launch with HIP events on the solver's stream (slower; for roofline reports) */
int qn_solver_set_profiling(qn_solver* s, int on);
/* 0 = pipelined (device-resident control, no host sync per decision; default for memoised device objectives),
 * 1 = synchronous (host reads the control block after every step; always used with host oracles / callbacks) */
int qn_solver_set_sync_mode(qn_solver* s, int sync);
/* tuning of the fused ROW kernels: rows per workgroup tile (2, 4, 8 or 16), column splits (1 .. 64); 0 keeps what is set.  (ABI <= 4 also took
 * negative `rows_per_block` codes that selected diagnostic paths: those are the named options below since ABI 5.) */
int qn_solver_set_tiling(qn_solver* s, int rows_per_block, int col_splits);
/* Named options (ABI 5).  None of them is needed to USE the library -- the reference has no counterpart: ls_solver.rs:66-111 takes a solver, a line
 * search and a closure -- they select, for tests and measurements, a path the library would not take by itself, or switch a step of the default path
 * off.  value != 0 switches the named thing ON, 0 OFF; [default] in brackets.  Unknown option: QN_ERROR_INPUT_PARAMS. */
typedef enum {
    QN_OPT_GENERIC_KERNELS = 1,            /* [0] the generic path: every O(n) vector operation in the one-workgroup control kernel, synchronous requests */
    QN_OPT_DEFERRED_UPDATE_STEP = 2,       /* [1] fused row kernels: the accepting step also opens the next line search (one launch less per iteration) */
    QN_OPT_SYMMETRIC_STORAGE = 3,          /* [1] stream only the upper block triangle of H and Q; 0: the fused ROW kernels on the full matrices */
    QN_OPT_SECOND_GENERATION = 4,          /* [1] the state machine in every kernel's prologue (5 launches per iteration); 0: first-generation tile kernels */
    QN_OPT_FOLDED_ACCEPT_REDUCE = 5,       /* [0] the accept-reduce inside the update-tile launch (n <= 4096; measured neutral) */
    QN_OPT_ROW_SLIVERS = 6,                /* [1] left-over diagonal tiles cut into 8-row slivers, one per workgroup (n = 4096); 0: whole tiles only */
    QN_OPT_EVAL_PAIR_INSTANCE = 7,         /* [1] the evaluation kernel's two-items-and-a-sliver instance where the work lists allow it; 0: the general body */
    QN_OPT_EVAL_MOVER_MULTIPLIER = 8,      /* [1] ... as mover + multiplier waves (round 6, csrc/qn_sym2r.hip.h); 0: round 5's kernel -- the same bits */
    QN_OPT_TAIL_REDUCE = 9,                /* [0] the update-reduce in the tail of the update-tile launch (bit-identical, measured slower) */
    QN_OPT_BOUNDED_SECOND_GENERATION = 10, /* [1] BFGSB / DFPB / SR1B with More-Thuente(B) on the second-generation path; 0: the generic path */
    QN_OPT_NEWTON_PIVOTED_LU = 11,         /* [0] Newton: the pivoted LU the reference's try_inverse stands for (newton/mod.rs:31-40) even for an SPD Hessian */
    QN_OPT_LU_PER_COLUMN_PANEL = 12,       /* [0] ... its panel with two launches per column (rounds 1-2) */
    QN_OPT_LU_LOOKAHEAD = 13,              /* [1] ... look-ahead on a second stream; 0: one stream */
    QN_OPT_LU_ONE_LAUNCH_PANEL = 14,       /* [1] ... the panel and the substitution sweeps as one launch each; 0: one launch per sub-panel / block */
    QN_OPT_LU_FORCE_WAIT_EXPIRY = 15,      /* [0] ... every bounded wait of the one-launch kernels expires at once (exercises the fallback) */
    QN_OPT_CHUNKS_PER_TRIP = 16,           /* [1] fused ROW kernels: column chunks per loop trip (1, 2 or 4) */
    QN_OPT_LU_SPLIT_ROLE_A = 17,           /* [4] ... the one-launch panel's pivot chain shared by 1 (0 too), 2 or 4 workgroups of one XCD (csrc/qn_lu_split.hip.h) -- the same bits */
    QN_OPT_LU_SPLIT_MIN_ROWS = 18,         /* [4160] ... for panels of at least `value` rows (a NUMBER, not a switch; shorter panels: one workgroup) */
    QN_OPT_BTB_PROJECT_IN_EVAL = 19,       /* [1] BackTrackingB on the second-generation path: the trial point projected inside the evaluation kernel (n = 4096's mover + multiplier kernel); 0: a projection launch per trial -- the same bits */
    QN_OPT_EVAL_ZIGZAG = 20,               /* [1] the mover + multiplier kernel streams its two tiles in the other order in launches of odd parity: an evaluation launch right behind another one starts with the tile the XCD's L2 still holds (csrc/qn_sym2r.hip.h, ZIG-ZAG); 0: the same order in every launch -- the same bits */
    QN_OPT_TOUCH_H_ROWS = 21,              /* [8] n = 4096: the accept-reduce launch carries workgroups that only load the first `value` rows (of a wave's 16; 0, 4, 6, 8, 10, 12 or 16) of the tile the update-tile launch's workgroup of the same index streams first -- into the L2 of the XCD both run on (csrc/qn_sym2.hip.h, TOUCH WORKGROUPS); a NUMBER; loads only -- the same bits */
    QN_OPT_TOUCH_Q_ROWS = 22,              /* [6] ... and the update-reduce launch for the evaluation launch behind it (rows of Q's tiles) */
    QN_OPT_PNEWTON_REUSE_FACTOR = 23,      /* [1] ProjectedNewton / SpectralProjectedNewton on a device quadratic: the Hessian's Cholesky factor is kept between iterations (the matrix does not change); 0: factorise in every iteration -- the same bits */
    QN_OPT_PNORM_NONTEMPORAL = 24,         /* [-1] PnormDescent: inverse_p through non-temporal loads; 1 / 0 force it on / off, -1 (a NUMBER): by size -- on once the matrix is past the Infinity Cache's reach (~230 MB, n ~ 5400) -- the same bits */
    QN_OPT_PNORM_ROWS_PER_WAVE = 25,       /* [0] ... rows a wave of its direction kernel holds in flight: 2 or 4 (a NUMBER); 0: by size (2 up to n = 8192) -- the same bits */
    QN_OPT_LBFGS_UNIT_SCALING = 26,        /* [0] L-BFGS: gamma = 1 in every iteration (H0 = I): the iterates of dense BFGS from H = I while no pair has been dropped */
    QN_OPT_MACHINE_FAST_STEPS = 27,        /* [1] second-generation path: the accept-reduce's and the update tiles' prologues run the steady iteration's step of the state machine as straight-line code in front of the generic machine (csrc/qn_sym2.hip.h, qn_s2_fast_step); 0: the generic machine alone -- the same bits */
    QN_OPT_HPASS_STORE_SKIP = 28           /* [1] second-generation path, one rank, BFGS / DFP unbounded, without the folded accept-reduce and the tail reduce: an update pass that finds ONE update pending applies it in registers and does not store H; the next pass applies that update and the newer one to the stored H and stores (csrc/qn_sym2.hip.h, s2_hpass_kernel; qn_stats.n_hpass_nostore, h_bytes_moved); 0: every pass stores -- the same bits.  Read once per qn_minimize call */
} qn_option;
int qn_solver_set_option(qn_solver* s, int option, int value);

/* ---------------------------------------------------------------------------------------------
 * Thin kernel-level FFI (what a Rust host loop would bind if it keeps `minimize` in Rust):
 * the BLAS-2 / rank-2 / vector primitives as individual calls on device buffers.
 * ------------------------------------------------------------------------------------------- */
int qn_dev_alloc(qn_context* ctx, size_t bytes, void** out_dev);
int qn_dev_free(qn_context* ctx, void* dev);
int qn_h2d(qn_context* ctx, void* dst_dev, const void* src_host, size_t bytes);
int qn_d2h(qn_context* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* y = A x for `nrows` rows of a row-major matrix with leading dimension ld (bfgs.rs:47 H*g, dfp.rs:118 H*y) */
int qn_gemv(qn_context* ctx, const double* a_dev, size_t ld, size_t nrows, size_t ncols, const double* x_dev, double* y_dev);
/* H_rows += c_su (s u' + u s') + c_ss s s' + c_uu u u' on rows [row0,row0+nrows) (bfgs.rs:115-124, dfp.rs:115-120) */
int qn_rank2_update(qn_context* ctx, double* h_dev, size_t ld, size_t row0, size_t nrows, size_t n, const double* s_dev,
                    const double* u_dev, double c_ss, double c_su, double c_uu);
/* out = x + t*d, two roundings per element (ls_solver.rs:60, bfgs.rs:94, backtracking.rs:32, morethuente.rs:182) */
int qn_axpy(qn_context* ctx, size_t n, const double* x_dev, double t, const double* d_dev, double* out_dev);
int qn_dot(qn_context* ctx, size_t n, const double* a_dev, const double* b_dev, double* out_host);  /* mod.rs:35,47,55 */
int qn_nrm2(qn_context* ctx, size_t n, const double* a_dev, double* out_host);                      /* bfgs.rs:74,97,99 */

#ifdef __cplusplus
}
#endif
#endif /* QN_HIP_H */
