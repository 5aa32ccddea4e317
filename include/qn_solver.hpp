// qn_solver.hpp -- header-only C++17 host mirror of the reference's trait surface over the C ABI (qn_hip.h).
//
// The reference is a compiled (Rust) crate; this is the compiled-language host side a user would write
// against: same names, argument meaning and error behaviour as the crate, so code reads like the reference's
// examples and tests.  Nothing numeric happens here -- every call forwards to libqn_hip.so (GPU only).
//
//   reference (Rust)                                   here (C++)
//   BFGS::new(tol, x0)                                 BFGS::new_(tol, x0)            bfgs.rs:27-39
//   DFP::new / GradientDescent::new                    DFP::new_ / GradientDescent::new_
//   MoreThuente::default().with_c1(..)                 MoreThuente::default_().with_c1(..)   morethuente.rs:16-62
//   BackTracking::new(c1, beta)                        BackTracking::new_(c1, beta)   backtracking.rs:8-10
//   FuncEvalMultivariate::new(f, g)                    FuncEvalMultivariate(f, g)     func_eval.rs:4-41
//   solver.minimize(&mut ls, oracle, a, b, callback)   solver.minimize(ls, oracle, a, b, callback)  ls_solver.rs:66-111
//   Result<(), SolverError> / .unwrap()                Result / .unwrap() (throws SolverError)      ls_solver.rs:10-20
#pragma once
#include <cmath>
#include <functional>
#include <optional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "qn_hip.h"

namespace optimization_solvers {

using Floating = double;                 // number.rs:3
using DVector = std::vector<Floating>;   // nalgebra::DVector<f64>

// ls_solver.rs:10-20
struct SolverError : std::runtime_error {
    enum Kind { MaxIterReached = QN_MAX_ITER_REACHED, OutOfDomain = QN_OUT_OF_DOMAIN, ErrorInputParams = QN_ERROR_INPUT_PARAMS,
                AbnormalTermination = QN_ABNORMAL_TERMINATION };
    Kind kind;
    explicit SolverError(int code, const std::string& detail = "")
        : std::runtime_error(std::string(qn_status_string(code)) + (detail.empty() ? "" : ": " + detail)), kind(static_cast<Kind>(code)) {}
};

// Result<(), SolverError>
class Result {
    std::optional<SolverError> err_;
  public:
    Result() = default;
    explicit Result(SolverError e) : err_(std::move(e)) {}
    bool is_ok() const { return !err_; }
    bool is_err() const { return bool(err_); }
    const SolverError& unwrap_err() const { return *err_; }
    void unwrap() const { if (err_) throw *err_; }
};

inline Result make_result(int status) {
    if (status == QN_OK) return Result();
    const bool detail = status == QN_ERROR_INPUT_PARAMS || status == QN_ABNORMAL_TERMINATION;
    return Result(SolverError(status, detail ? qn_last_error_message() : ""));
}
inline void check(int status) { make_result(status).unwrap(); }

// func_eval.rs:4-41
class FuncEvalMultivariate {
    Floating f_;
    DVector g_;
    std::optional<DVector> hessian_; // column-major n x n, like DMatrix (func_eval.rs:8)
  public:
    FuncEvalMultivariate(Floating f, DVector g) : f_(f), g_(std::move(g)) {}
    const Floating& f() const { return f_; }
    const DVector& g() const { return g_; }
    FuncEvalMultivariate with_hessian(DVector h_colmajor) && { hessian_ = std::move(h_colmajor); return std::move(*this); } // func_eval.rs:27-30
    const std::optional<DVector>& hessian() const { return hessian_; }
};

// one GPU (optionally one rank of a row-sharded group)
class Context {
    qn_context* h_ = nullptr;
  public:
    explicit Context(int device = 0) { check(qn_context_create(device, &h_)); }
    Context(int device, int rank, int world, const void* unique_id) { check(qn_context_create_sharded(device, rank, world, unique_id, &h_)); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ~Context() { qn_context_destroy(h_); }
    qn_context* handle() const { return h_; }
    static Context& default_context() { static Context c(0); return c; }
};

// LineSearch::compute_step_len (line_search/mod.rs:14-23) for a line-search mirror `LS` and a host closure
template <class LS, class Oracle>
inline Floating compute_step_len(LS& ls, const DVector& x_k, const FuncEvalMultivariate& eval_x_k, const DVector& direction_k, Oracle&& oracle,
                                 size_t max_iter, Context& ctx = Context::default_context()) {
    using OracleT = std::remove_reference_t<Oracle>;
    OracleT* op = &oracle;
    auto tramp = [](void* user, const double* x, size_t n, double* f, double* g) -> int {
        DVector xv(x, x + n);
        FuncEvalMultivariate ev = (*static_cast<OracleT*>(user))(xv);
        *f = ev.f();
        for (size_t i = 0; i < n; ++i) g[i] = ev.g()[i];
        return 0;
    };
    qn_oracle o{};
    o.kind = QN_ORACLE_HOST;
    o.memoize = 0;
    o.host_fn = tramp;
    o.host_user = op;
    Floating t = 0;
    check(qn_compute_step_len(ctx.handle(), &ls.ffi(), x_k.data(), eval_x_k.f(), eval_x_k.g().data(), direction_k.data(), x_k.size(), &o, max_iter, &t));
    return t;
}

// morethuente.rs:6-62
class MoreThuente {
    qn_linesearch s_;
  public:
    template <class Oracle>
    Floating compute_step_len(const DVector& x_k, const FuncEvalMultivariate& eval_x_k, const DVector& direction_k, Oracle&& oracle, size_t max_iter) {
        return optimization_solvers::compute_step_len(*this, x_k, eval_x_k, direction_k, oracle, max_iter);
    }
    MoreThuente() { qn_morethuente_default(&s_); }
    static MoreThuente default_() { return MoreThuente(); }
    MoreThuente with_deltas(Floating dmin, Floating d, Floating dmax) && { check(qn_morethuente_with_deltas(&s_, dmin, d, dmax)); return *this; }
    MoreThuente with_t_min(Floating v) && { check(qn_morethuente_with_t_min(&s_, v)); return *this; }
    MoreThuente with_t_max(Floating v) && { check(qn_morethuente_with_t_max(&s_, v)); return *this; }
    MoreThuente with_c1(Floating v) && { check(qn_morethuente_with_c1(&s_, v)); return *this; } // assert!s -> ErrorInputParams
    MoreThuente with_c2(Floating v) && { check(qn_morethuente_with_c2(&s_, v)); return *this; }
    Floating c1() const { return s_.c1; }
    Floating c2() const { return s_.c2; }
    Floating t_max() const { return s_.t_max; }
    qn_linesearch& ffi() { return s_; }
};

// backtracking.rs:3-11
class BackTracking {
    qn_linesearch s_;
  public:
    template <class Oracle>
    Floating compute_step_len(const DVector& x_k, const FuncEvalMultivariate& eval_x_k, const DVector& direction_k, Oracle&& oracle, size_t max_iter) {
        return optimization_solvers::compute_step_len(*this, x_k, eval_x_k, direction_k, oracle, max_iter);
    }
    BackTracking(Floating c1, Floating beta) { qn_backtracking_new(&s_, c1, beta); }
    static BackTracking new_(Floating c1, Floating beta) { return BackTracking(c1, beta); }
    qn_linesearch& ffi() { return s_; }
};

// gll_quadratic.rs: the non-monotone search for SpectralProjectedGradient / ProjectedGradientDescent (the history lives in the solver)
// line_search/nosearch.rs: compute_step_len returns 1.0 and never calls the oracle; pairs with GradientDescent, Newton, CoordinateDescent, PnormDescent
class NoSearch {
    qn_linesearch s_;
  public:
    NoSearch() { qn_nosearch_new(&s_); }
    qn_linesearch& ffi() { return s_; }
};

class GLLQuadratic {
    qn_linesearch s_;
  public:
    template <class Oracle>
    Floating compute_step_len(const DVector& x_k, const FuncEvalMultivariate& eval_x_k, const DVector& direction_k, Oracle&& oracle, size_t max_iter) {
        return optimization_solvers::compute_step_len(*this, x_k, eval_x_k, direction_k, oracle, max_iter);
    }
    GLLQuadratic(Floating c1, size_t m) { qn_gll_quadratic_new(&s_, c1, m); }
    static GLLQuadratic new_(Floating c1, size_t m) { return GLLQuadratic(c1, m); }
    GLLQuadratic with_sigmas(Floating sigma1, Floating sigma2) && { qn_gll_quadratic_with_sigmas(&s_, sigma1, sigma2); return *this; }
    Floating c1() const { return s_.c1; }
    qn_linesearch& ffi() { return s_; }
};

// StrongWolfe (QN_LS_STRONG_WOLFE): MINPACK-2 dcsrch for the O(n) solvers (SPG, projected gradient, the projected Newton pair, LBFGS / ProjectedLBFGS, NonlinearCG),
// one oracle call per trial; with a box of its own every search's stpmax is clipped to it (t_max itself is never modified).  0 < c1 < c2 < 1 is
// checked by minimize.  Keeps its own copies of the bounds.
class StrongWolfe {
    qn_linesearch s_;
    DVector lb_, ub_;
    void rebind() {
        if (!lb_.empty()) qn_linesearch_with_lower_bound(&s_, lb_.data());
        if (!ub_.empty()) qn_linesearch_with_upper_bound(&s_, ub_.data());
    }
  public:
    explicit StrongWolfe(Floating c1 = 1e-4, Floating c2 = 0.9) { qn_strong_wolfe_new(&s_, c1, c2); }
    StrongWolfe(const StrongWolfe& o) : s_(o.s_), lb_(o.lb_), ub_(o.ub_) { rebind(); }
    StrongWolfe& operator=(const StrongWolfe& o) { s_ = o.s_; lb_ = o.lb_; ub_ = o.ub_; rebind(); return *this; }
    static StrongWolfe new_(Floating c1 = 1e-4, Floating c2 = 0.9) { return StrongWolfe(c1, c2); }
    StrongWolfe with_xtol(Floating v) && { check(qn_strong_wolfe_with_xtol(&s_, v)); return *this; }
    StrongWolfe with_t_min(Floating v) && { check(qn_morethuente_with_t_min(&s_, v)); return *this; }
    StrongWolfe with_t_max(Floating v) && { check(qn_morethuente_with_t_max(&s_, v)); return *this; }
    StrongWolfe with_lower_bound(const DVector& lb) && { lb_ = lb; rebind(); return *this; }
    StrongWolfe with_upper_bound(const DVector& ub) && { ub_ = ub; rebind(); return *this; }
    Floating c1() const { return s_.c1; }
    Floating c2() const { return s_.c2; }
    Floating xtol() const { return s_.delta; }
    Floating t_max() const { return s_.t_max; }
    qn_linesearch& ffi() { return s_; }
};

// ExactQuadratic (QN_LS_EXACT_QUADRATIC): the exact step -g.d / d'Qd on a device quadratic (Quadratic, SparseQuadratic) for SpectralProjectedGradient,
// ProjectedGradientDescent, LBFGS / ProjectedLBFGS and NonlinearCG -- with the last, linear conjugate gradients.  refresh_every = 1: the objective
// evaluates every accepted point; k > 1: every k-th; 0: never, except that convergence is only declared on a gradient the objective evaluated.
class ExactQuadratic {
    qn_linesearch s_;
  public:
    explicit ExactQuadratic(int refresh_every = 1) { qn_exact_quadratic_new(&s_, refresh_every); }
    static ExactQuadratic new_(int refresh_every = 1) { return ExactQuadratic(refresh_every); }
    int refresh_every() const { return s_._pad; }
    qn_linesearch& ffi() { return s_; }
};

// what ExactQuadratic did in the last minimize (qn_solver_exact_state)
struct ExactState {
    size_t curvature_passes = 0, refreshes = 0;
    Floating last_t = 0, last_curvature = 0;
};

// backtracking_b.rs: projected trial points; keeps its own copies of the box
class BackTrackingB {
    qn_linesearch s_;
    DVector lb_, ub_;
  public:
    BackTrackingB(Floating c1, Floating beta, DVector lower_bound, DVector upper_bound) : lb_(std::move(lower_bound)), ub_(std::move(upper_bound)) {
        qn_backtracking_b_new(&s_, c1, beta, lb_.data(), ub_.data());
    }
    BackTrackingB(const BackTrackingB&) = delete; // (the struct points into lb_ / ub_)
    qn_linesearch& ffi() { return s_; }
};

// a device-resident objective (built-in quadratic f = 1/2 x'Qx - b'x)
class Quadratic {
    qn_objective* h_ = nullptr;
    size_t n_;
  public:
    Quadratic(const DVector& q_rowmajor, const DVector& b, Context& ctx = Context::default_context()) : n_(b.size()) {
        check(qn_quadratic_create(ctx.handle(), n_, q_rowmajor.data(), b.data(), &h_));
    }
    Quadratic(const Quadratic&) = delete;
    ~Quadratic() { qn_objective_destroy(h_); }
    qn_objective* handle() const { return h_; }
    FuncEvalMultivariate operator()(const DVector& x) const {
        DVector g(n_);
        Floating f = 0;
        check(qn_objective_eval(h_, x.data(), &f, g.data()));
        return FuncEvalMultivariate(f, std::move(g));
    }
    DVector hessian(const DVector& x) const { // column-major n x n: Q itself
        DVector h(n_ * n_);
        check(qn_objective_hessian(h_, x.data(), h.data()));
        return h;
    }
    std::pair<DVector, Floating> hess_vec(const DVector& v) const { // (Q v, v'Qv): one pass over Q, no evaluation of f
        if (v.size() != n_) throw SolverError{SolverError::ErrorInputParams, "v does not have the objective's n entries"};
        DVector q(n_);
        Floating c = 0;
        check(qn_objective_hess_vec(h_, v.data(), q.data(), &c));
        return {std::move(q), c};
    }
    std::pair<DVector, Floating> hess_vec_at(const DVector&, const DVector& v) const { return hess_vec(v); } // the Hessian is Q wherever x is
};

// a device-resident objective f = log sum_i exp(a_i'x + c_i) + mu/2 ||x||^2 (A is m x n row-major).  Newton forms its Hessian on the device.
class LogSumExp {
    qn_objective* h_ = nullptr;
    size_t n_;
  public:
    LogSumExp(const DVector& a_rowmajor, const DVector& c, size_t n, Floating mu, Context& ctx = Context::default_context()) : n_(n) {
        check(qn_logsumexp_create(ctx.handle(), c.size(), n, a_rowmajor.data(), c.data(), mu, &h_));
    }
    LogSumExp(const LogSumExp&) = delete;
    ~LogSumExp() { qn_objective_destroy(h_); }
    qn_objective* handle() const { return h_; }
    FuncEvalMultivariate operator()(const DVector& x) const {
        DVector g(n_);
        Floating f = 0;
        check(qn_objective_eval(h_, x.data(), &f, g.data()));
        return FuncEvalMultivariate(f, std::move(g));
    }
    DVector hessian(const DVector& x) const { // column-major n x n, A'(diag(p) - p p')A + mu I from the device kernel
        DVector h(n_ * n_);
        check(qn_objective_hessian(h_, x.data(), h.data()));
        return h;
    }
    std::pair<DVector, Floating> hess_vec_at(const DVector& x, const DVector& v) const { // (H(x) v, v'H(x)v): the weights at x, then one stream of A; no matrix
        if (x.size() != n_ || v.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x or v does not have the objective's n entries"};
        DVector q(n_);
        Floating c = 0;
        check(qn_objective_hess_vec_at(h_, x.data(), v.data(), q.data(), &c));
        return {std::move(q), c};
    }
    DVector hess_diag_at(const DVector& x) const { // diag H(x): the weights at x, then one pass over A with squared entries; no matrix
        if (x.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x does not have the objective's n entries"};
        DVector d(n_);
        check(qn_objective_hess_diag_at(h_, x.data(), d.data()));
        return d;
    }
};

// a device-resident regularised logistic regression, f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2 (A is m x n row-major and dense).  y_i is
// exactly -1 or +1 (0 / 1 labels: pass 2 y - 1; anything else throws ErrorInputParams); weights are >= 0, a row with weight 0 is masked (the value is
// that of the problem with the row deleted); an empty `weights`: all ones.  It runs under SpectralProjectedGradient, ProjectedGradientDescent, LBFGS /
// ProjectedLBFGS, NonlinearCG and NewtonCG.
class Logistic {
    qn_objective* h_ = nullptr;
    size_t n_;
  public:
    Logistic(const DVector& a_rowmajor, const DVector& y, size_t n, Floating mu, const DVector& weights = DVector(), Context& ctx = Context::default_context()) : n_(n) {
        if (!weights.empty() && weights.size() != y.size()) throw SolverError{SolverError::ErrorInputParams, "weights does not have one entry per row"};
        if (a_rowmajor.size() != y.size() * n) throw SolverError{SolverError::ErrorInputParams, "a_rowmajor is not y.size() x n"};
        check(qn_logistic_create(ctx.handle(), y.size(), n, a_rowmajor.data(), y.data(), weights.empty() ? nullptr : weights.data(), mu, &h_));
    }
    Logistic(const Logistic&) = delete;
    ~Logistic() { qn_objective_destroy(h_); }
    qn_objective* handle() const { return h_; }
    FuncEvalMultivariate operator()(const DVector& x) const {
        DVector g(n_);
        Floating f = 0;
        check(qn_objective_eval(h_, x.data(), &f, g.data()));
        return FuncEvalMultivariate(f, std::move(g));
    }
    std::pair<DVector, Floating> hess_vec_at(const DVector& x, const DVector& v) const { // (H(x) v, v'H(x)v), H = A' diag(d) A + mu I: d at x (one pass of A), then one stream of A; no matrix
        if (x.size() != n_ || v.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x or v does not have the objective's n entries"};
        DVector q(n_);
        Floating c = 0;
        check(qn_objective_hess_vec_at(h_, x.data(), v.data(), q.data(), &c));
        return {std::move(q), c};
    }
    DVector hess_diag_at(const DVector& x) const { // diag H(x): the weights at x, then one pass over A with squared entries; no matrix
        if (x.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x does not have the objective's n entries"};
        DVector d(n_);
        check(qn_objective_hess_diag_at(h_, x.data(), d.data()));
        return d;
    }
};

// the same logistic regression with a sparse A in CSR (m x n, the columns of a row strictly increasing) and no limit on n: the device keeps A and A'
// (24 bytes per nonzero), so the transpose product uses no atomics and every sum has one fixed order.  Labels, weights and mu as Logistic's.  It runs
// under SpectralProjectedGradient, ProjectedGradientDescent, LBFGS / ProjectedLBFGS, NonlinearCG and NewtonCG.  Index: int32_t or int64_t, for both arrays.
class SparseLogistic {
    qn_objective* h_ = nullptr;
    size_t n_;
  public:
    template <class Index>
    SparseLogistic(const std::vector<Index>& indptr, const std::vector<Index>& indices, const DVector& data, const DVector& y, size_t n, Floating mu,
                   const DVector& weights = DVector(), Context& ctx = Context::default_context()) : n_(n) {
        static_assert(sizeof(Index) == 4 || sizeof(Index) == 8, "CSR indices are 32 or 64 bits wide");
        if (indptr.size() != y.size() + 1 || indices.size() != data.size()) throw SolverError{SolverError::ErrorInputParams, "CSR arrays do not match"};
        if (!weights.empty() && weights.size() != y.size()) throw SolverError{SolverError::ErrorInputParams, "weights does not have one entry per row"};
        const Index no_index = 0; // (an empty matrix: the library takes a null pointer for a missing argument)
        const Floating no_value = 0;
        check(qn_sparse_logistic_create(ctx.handle(), y.size(), n, data.size(), indptr.data(), indices.empty() ? &no_index : indices.data(), (int)sizeof(Index),
                                        data.empty() ? &no_value : data.data(), y.data(), weights.empty() ? nullptr : weights.data(), mu, &h_));
    }
    SparseLogistic(const SparseLogistic&) = delete;
    ~SparseLogistic() { qn_objective_destroy(h_); }
    qn_objective* handle() const { return h_; }
    FuncEvalMultivariate operator()(const DVector& x) const {
        if (x.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x does not have the objective's n entries"};
        DVector g(n_);
        Floating f = 0;
        check(qn_objective_eval(h_, x.data(), &f, g.data()));
        return FuncEvalMultivariate(f, std::move(g));
    }
    std::pair<DVector, Floating> hess_vec_at(const DVector& x, const DVector& v) const { // (H(x) v, v'H(x)v), H = A' diag(d) A + mu I: a weights pass at x, then the product's two passes; no matrix
        if (x.size() != n_ || v.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x or v does not have the objective's n entries"};
        DVector q(n_);
        Floating c = 0;
        check(qn_objective_hess_vec_at(h_, x.data(), v.data(), q.data(), &c));
        return {std::move(q), c};
    }
    DVector hess_diag_at(const DVector& x) const { // diag H(x): the weights at x, then one pass over A with squared entries; no matrix
        if (x.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x does not have the objective's n entries"};
        DVector d(n_);
        check(qn_objective_hess_diag_at(h_, x.data(), d.data()));
        return d;
    }
    void set_lanes(int rows, int cols) { check(qn_sparse_logistic_set_lanes(h_, rows, cols)); } // 0: automatic
    size_t nnz() const { size_t v = 0; check(qn_sparse_logistic_info(h_, &v, nullptr, nullptr, nullptr, nullptr)); return v; }
    size_t n_long_rows() const { size_t v = 0; check(qn_sparse_logistic_info(h_, nullptr, nullptr, nullptr, &v, nullptr)); return v; }
    size_t n_long_cols() const { size_t v = 0; check(qn_sparse_logistic_info(h_, nullptr, nullptr, nullptr, nullptr, &v)); return v; }
};

// a device-resident regularised softmax (multinomial logistic) regression on a dense A (m x n row-major): labels in {0, .., n_classes - 1} (anything
// else throws ErrorInputParams), weights >= 0 (a 0 masks its row; empty: all ones).  The parameter vector is CLASS-MAJOR, x[k n + j] = W[k, j], with
// N = n_classes * n entries: that is the dimension a solver is created with.  It runs under SpectralProjectedGradient, ProjectedGradientDescent,
// LBFGS / ProjectedLBFGS, NonlinearCG and NewtonCG.
class Multinomial {
    qn_objective* h_ = nullptr;
    size_t n_, k_;
  public:
    Multinomial(const DVector& a_rowmajor, const std::vector<int32_t>& labels, size_t n, size_t n_classes, Floating mu, const DVector& weights = DVector(),
                Context& ctx = Context::default_context()) : n_(n * n_classes), k_(n_classes) {
        if (!weights.empty() && weights.size() != labels.size()) throw SolverError{SolverError::ErrorInputParams, "weights does not have one entry per row"};
        if (a_rowmajor.size() != labels.size() * n) throw SolverError{SolverError::ErrorInputParams, "a_rowmajor is not labels.size() x n"};
        check(qn_multinomial_create(ctx.handle(), labels.size(), n, n_classes, a_rowmajor.data(), labels.data(), weights.empty() ? nullptr : weights.data(), mu, &h_));
    }
    Multinomial(const Multinomial&) = delete;
    ~Multinomial() { qn_objective_destroy(h_); }
    qn_objective* handle() const { return h_; }
    size_t n_classes() const { return k_; }
    size_t size() const { return n_; } // N = n_classes * n
    void set_kernel(int kernel) { check(qn_multinomial_set_kernel(h_, kernel)); } // 0: automatic, 1: register-blocked, 2: MFMA (K <= 64 where built)
    FuncEvalMultivariate operator()(const DVector& x) const {
        DVector g(n_);
        Floating f = 0;
        check(qn_objective_eval(h_, x.data(), &f, g.data()));
        return FuncEvalMultivariate(f, std::move(g));
    }
    std::pair<DVector, Floating> hess_vec_at(const DVector& x, const DVector& v) const { // (H(x) v, v'H(x)v): P at x (one pass of A), then one stream of A; no matrix
        if (x.size() != n_ || v.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x or v does not have the objective's N entries"};
        DVector q(n_);
        Floating c = 0;
        check(qn_objective_hess_vec_at(h_, x.data(), v.data(), q.data(), &c));
        return {std::move(q), c};
    }
};

// the same softmax regression with a sparse A in CSR (m x n, the columns of a row strictly increasing) and no limit on n_classes * n: the device keeps
// A and A' (24 bytes per nonzero) and feature-major copies of the class-major vectors, so both halves of an evaluation are a sparse matrix times a
// skinny dense one, with no atomics and every sum in one fixed order.  Labels, weights, mu and the CLASS-MAJOR parameter vector as Multinomial's.  It
// runs under SpectralProjectedGradient, ProjectedGradientDescent, LBFGS / ProjectedLBFGS, NonlinearCG and NewtonCG.  Index: int32_t or int64_t.
class SparseMultinomial {
    qn_objective* h_ = nullptr;
    size_t n_, k_, m_;
  public:
    template <class Index>
    SparseMultinomial(const std::vector<Index>& indptr, const std::vector<Index>& indices, const DVector& data, const std::vector<int32_t>& labels, size_t n,
                      size_t n_classes, Floating mu, const DVector& weights = DVector(), Context& ctx = Context::default_context())
        : n_(n * n_classes), k_(n_classes), m_(labels.size()) {
        static_assert(sizeof(Index) == 4 || sizeof(Index) == 8, "CSR indices are 32 or 64 bits wide");
        if (indptr.size() != labels.size() + 1 || indices.size() != data.size()) throw SolverError{SolverError::ErrorInputParams, "CSR arrays do not match"};
        if (!weights.empty() && weights.size() != labels.size()) throw SolverError{SolverError::ErrorInputParams, "weights does not have one entry per row"};
        const Index no_index = 0; // (an empty matrix: the library takes a null pointer for a missing argument)
        const Floating no_value = 0;
        check(qn_sparse_multinomial_create(ctx.handle(), labels.size(), n, n_classes, data.size(), indptr.data(), indices.empty() ? &no_index : indices.data(),
                                           (int)sizeof(Index), data.empty() ? &no_value : data.data(), labels.data(), weights.empty() ? nullptr : weights.data(), mu, &h_));
    }
    SparseMultinomial(const SparseMultinomial&) = delete;
    ~SparseMultinomial() { qn_objective_destroy(h_); }
    qn_objective* handle() const { return h_; }
    size_t n_classes() const { return k_; }
    size_t size() const { return n_; } // N = n_classes * n
    FuncEvalMultivariate operator()(const DVector& x) const {
        if (x.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x does not have the objective's N entries"};
        DVector g(n_);
        Floating f = 0;
        check(qn_objective_eval(h_, x.data(), &f, g.data()));
        return FuncEvalMultivariate(f, std::move(g));
    }
    std::pair<DVector, Floating> hess_vec_at(const DVector& x, const DVector& v) const { // (H(x) v, v'H(x)v): a weights pass at x, then the product's five launches; no matrix
        if (x.size() != n_ || v.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x or v does not have the objective's N entries"};
        DVector q(n_);
        Floating c = 0;
        check(qn_objective_hess_vec_at(h_, x.data(), v.data(), q.data(), &c));
        return {std::move(q), c};
    }
    DVector probabilities(const DVector& x) const { // m x n_classes, row-major; a masked row's are zeros
        if (x.size() != n_) throw SolverError{SolverError::ErrorInputParams, "x does not have the objective's N entries"};
        DVector p(m_ * k_);
        check(qn_sparse_multinomial_probabilities(h_, x.data(), p.data()));
        return p;
    }
    void set_lanes(int rows, int cols) { check(qn_sparse_multinomial_set_lanes(h_, rows, cols)); } // 0: automatic
    size_t nnz() const { size_t v = 0; check(qn_sparse_multinomial_info(h_, &v, nullptr, nullptr, nullptr, nullptr, nullptr)); return v; }
    size_t n_long_rows() const { size_t v = 0; check(qn_sparse_multinomial_info(h_, nullptr, nullptr, nullptr, &v, nullptr, nullptr)); return v; }
    size_t n_long_cols() const { size_t v = 0; check(qn_sparse_multinomial_info(h_, nullptr, nullptr, nullptr, nullptr, &v, nullptr)); return v; }
    int kp() const { int v = 0; check(qn_sparse_multinomial_info(h_, nullptr, nullptr, nullptr, nullptr, nullptr, &v)); return v; }
};

// a device-resident objective f = 1/2 x'Qx - b'x with a sparse Q in CSR (both triangles of a symmetric matrix): the large objective of the O(n)
// solvers -- SpectralProjectedGradient, ProjectedGradientDescent, LBFGS / ProjectedLBFGS.  Index: int32_t or int64_t, for both arrays.
class SparseQuadratic {
    qn_objective* h_ = nullptr;
    size_t n_;
    template <class Index>
    void create(const std::vector<Index>& indptr, const std::vector<Index>& indices, const DVector& data, const DVector& b, Context& ctx) {
        static_assert(sizeof(Index) == 4 || sizeof(Index) == 8, "CSR indices are 32 or 64 bits wide");
        if (indptr.size() != n_ + 1 || indices.size() != data.size()) throw SolverError{SolverError::ErrorInputParams, "CSR arrays do not match n / nnz"};
        const Index none = 0; // (an empty matrix: data() of an empty vector may be null, which the library takes for a missing argument)
        const Floating zero = 0;
        check(qn_sparse_quadratic_create(ctx.handle(), n_, data.size(), indptr.data(), indices.empty() ? &none : indices.data(), (int)sizeof(Index),
                                         data.empty() ? &zero : data.data(), b.data(), &h_));
    }
  public:
    SparseQuadratic(const std::vector<int32_t>& indptr, const std::vector<int32_t>& indices, const DVector& data, const DVector& b,
                    Context& ctx = Context::default_context()) : n_(b.size()) { create(indptr, indices, data, b, ctx); }
    SparseQuadratic(const std::vector<int64_t>& indptr, const std::vector<int64_t>& indices, const DVector& data, const DVector& b,
                    Context& ctx = Context::default_context()) : n_(b.size()) { create(indptr, indices, data, b, ctx); }
    SparseQuadratic(const SparseQuadratic&) = delete;
    ~SparseQuadratic() { qn_objective_destroy(h_); }
    qn_objective* handle() const { return h_; }
    FuncEvalMultivariate operator()(const DVector& x) const {
        DVector g(n_);
        Floating f = 0;
        check(qn_objective_eval(h_, x.data(), &f, g.data()));
        return FuncEvalMultivariate(f, std::move(g));
    }
    std::pair<DVector, Floating> hess_vec(const DVector& v) const { // (Q v, v'Qv): the CSR kernel's curvature form, one pass over Q
        if (v.size() != n_) throw SolverError{SolverError::ErrorInputParams, "v does not have the objective's n entries"};
        DVector q(n_);
        Floating c = 0;
        check(qn_objective_hess_vec(h_, v.data(), q.data(), &c));
        return {std::move(q), c};
    }
    std::pair<DVector, Floating> hess_vec_at(const DVector&, const DVector& v) const { return hess_vec(v); } // the Hessian is Q wherever x is
    size_t nnz() const { size_t v = 0; check(qn_objective_sparse_info(h_, &v, nullptr, nullptr, nullptr)); return v; }
    int lanes_per_row() const { int v = 0; check(qn_objective_sparse_info(h_, nullptr, &v, nullptr, nullptr)); return v; }
    size_t n_long_rows() const { size_t v = 0; check(qn_objective_sparse_info(h_, nullptr, nullptr, &v, nullptr)); return v; }
    bool symmetric() const { int v = 0; check(qn_objective_sparse_info(h_, nullptr, nullptr, nullptr, &v)); return v != 0; }
    void set_lanes_per_row(int lanes) { check(qn_sparse_quadratic_set_lanes_per_row(h_, lanes)); } // 0: chosen from the mean row length
};

template <int METHOD>
class LineSearchSolver { // ls_solver.rs:23-112 for the three solvers on the path
    qn_solver* h_ = nullptr;
    size_t n_;
    mutable DVector x_cache_;
    mutable size_t k_cache_ = 0;
    mutable std::optional<Floating> opt_cache_[2];
  public:
    using Self = LineSearchSolver<METHOD>;
    LineSearchSolver(Floating tol, const DVector& x0, Context& ctx = Context::default_context()) : n_(x0.size()) {
        check(qn_solver_create(ctx.handle(), METHOD, tol, x0.data(), x0.size(), &h_));
    }
    qn_solver* handle() const { return h_; }
    ExactState exact_state() const { // ExactQuadratic, of the last minimize (the first-order family's solvers)
        ExactState e;
        check(qn_solver_exact_state(h_, &e.curvature_passes, &e.refreshes, &e.last_t, &e.last_curvature));
        return e;
    }
    static Self new_(Floating tol, const DVector& x0) { return Self(tol, x0); }
    LineSearchSolver(const Self&) = delete;
    LineSearchSolver(Self&& o) noexcept : h_(o.h_), n_(o.n_) { o.h_ = nullptr; }
    ~LineSearchSolver() { if (h_) qn_solver_destroy(h_); }

    // getters generated by derive_getters (bfgs.rs:3-12) and LineSearchSolver::xk/k (bfgs.rs:52-63)
    const DVector& x() const { x_cache_.resize(n_); check(qn_solver_get_x(h_, x_cache_.data())); return x_cache_; }
    const DVector& xk() const { return x(); }
    const size_t& k() const { k_cache_ = qn_solver_k(h_); return k_cache_; }
    Floating tol() const { return qn_solver_tol(h_); }
    std::optional<Floating> s_norm() const { Floating v; int some; check(qn_solver_s_norm(h_, &v, &some)); return some ? std::optional<Floating>(v) : std::nullopt; }
    std::optional<Floating> y_norm() const { Floating v; int some; check(qn_solver_y_norm(h_, &v, &some)); return some ? std::optional<Floating>(v) : std::nullopt; }
    bool next_iterate_too_close() const { int v; check(qn_solver_next_iterate_too_close(h_, &v)); return v != 0; }                   // bfgs.rs:15-20
    bool gradient_next_iterate_too_close() const { int v; check(qn_solver_gradient_next_iterate_too_close(h_, &v)); return v != 0; } // bfgs.rs:21-26
    DVector approx_inv_hessian() const { DVector m(n_ * n_); check(qn_solver_get_inv_hessian(h_, m.data(), 1)); return m; }          // column-major, like DMatrix
    std::optional<Floating> decrement_squared() const { Floating v; int some; check(qn_solver_decrement_squared(h_, &v, &some)); return some ? std::optional<Floating>(v) : std::nullopt; } // newton/mod.rs:10
    bool has_converged(const FuncEvalMultivariate& eval) const { // bfgs.rs:64-76 / gradient_descent.rs:46-53
        if (METHOD == QN_NEWTON) { // newton/mod.rs:62-68: half the squared decrement of the last direction; false before the first
            const std::optional<Floating> d = decrement_squared();
            return d ? *d * 0.5 < tol() : false;
        }
        if (METHOD == QN_GRADIENT_DESCENT || METHOD == QN_COORDINATE_DESCENT || METHOD == QN_PNORM_DESCENT || METHOD == QN_NONLINEAR_CG || METHOD == QN_NEWTON_CG) { // (pnorm_descent.rs:52-59, coordinate_descent.rs:61-68)
            Floating acc = -INFINITY;
            for (Floating v : eval.g()) acc = std::fmax(std::fabs(v), acc);
            return acc < tol();
        }
        if (next_iterate_too_close() || gradient_next_iterate_too_close()) return true;
        Floating s = 0;
        for (Floating v : eval.g()) s += v * v;
        return std::sqrt(s) < tol();
    }

    // minimize with a host closure: the reference's exact oracle-call sequence (ls_solver.rs:66-111)
    // (a device objective is callable too: without the constraint a non-const Quadratic / LogSumExp lvalue would bind here, as a host closure)
    template <class LS, class Oracle, class = std::enable_if_t<!std::is_same_v<std::decay_t<Oracle>, Quadratic> && !std::is_same_v<std::decay_t<Oracle>, LogSumExp> &&
                                                               !std::is_same_v<std::decay_t<Oracle>, SparseQuadratic> && !std::is_same_v<std::decay_t<Oracle>, Logistic> &&
                                                               !std::is_same_v<std::decay_t<Oracle>, SparseLogistic> && !std::is_same_v<std::decay_t<Oracle>, Multinomial> &&
                                                               !std::is_same_v<std::decay_t<Oracle>, SparseMultinomial>>>
    Result minimize(LS& line_search, Oracle&& oracle, size_t max_iter_solver, size_t max_iter_line_search,
                    std::optional<std::function<void(const Self&)>> callback = std::nullopt) {
        using OracleT = std::remove_reference_t<Oracle>;
        struct Ctx { OracleT* o; size_t n; } octx{&oracle, n_};
        auto tramp = [](void* user, const double* x, size_t n, double* f, double* g) -> int {
            Ctx* c = static_cast<Ctx*>(user);
            DVector xv(x, x + n);
            FuncEvalMultivariate ev = (*c->o)(xv);
            *f = ev.f();
            for (size_t i = 0; i < n; ++i) g[i] = ev.g()[i];
            return 0;
        };
        struct Cb { Self* me; std::function<void(const Self&)>* f; } cb{this, callback ? &*callback : nullptr};
        auto cb_tramp = [](void* user, qn_solver*) { Cb* c = static_cast<Cb*>(user); (*c->f)(*c->me); };
        auto htramp = [](void* user, const double* x, size_t n, double* h) -> int { // the Hessian part of the FuncEval (Newton and the projected Newton solvers)
            Ctx* c = static_cast<Ctx*>(user);
            DVector xv(x, x + n);
            FuncEvalMultivariate ev = (*c->o)(xv);
            if (!ev.hessian() || ev.hessian()->size() != n * n) return 1; // "Hessian not available in the oracle"
            for (size_t i = 0; i < n * n; ++i) h[i] = (*ev.hessian())[i];
            return 0;
        };
        qn_oracle o{};
        o.kind = QN_ORACLE_HOST;
        o.memoize = 0;
        o.host_fn = tramp;
        o.host_user = &octx;
        if (METHOD == QN_NEWTON || METHOD == QN_PROJECTED_NEWTON || METHOD == QN_SPECTRAL_PROJECTED_NEWTON) o.host_hessian_fn = htramp;
        const int st = qn_minimize(h_, &line_search.ffi(), &o, max_iter_solver, max_iter_line_search,
                                   callback ? static_cast<qn_callback_fn>(cb_tramp) : nullptr, &cb);
        return make_result(st);
    }

    // minimize with a device-resident objective: no host round trip per oracle call, distinct points evaluated once
    template <class LS>
    Result minimize(LS& line_search, const Quadratic& objective, size_t max_iter_solver, size_t max_iter_line_search) {
        qn_oracle o{};
        o.kind = QN_ORACLE_OBJECTIVE;
        o.memoize = 1;
        o.objective = objective.handle();
        return make_result(qn_minimize(h_, &line_search.ffi(), &o, max_iter_solver, max_iter_line_search, nullptr, nullptr));
    }
    template <class LS>
    Result minimize(LS& line_search, const LogSumExp& objective, size_t max_iter_solver, size_t max_iter_line_search) {
        qn_oracle o{};
        o.kind = QN_ORACLE_OBJECTIVE;
        o.memoize = 1;
        o.objective = objective.handle();
        return make_result(qn_minimize(h_, &line_search.ffi(), &o, max_iter_solver, max_iter_line_search, nullptr, nullptr));
    }
    template <class LS>
    Result minimize(LS& line_search, const Logistic& objective, size_t max_iter_solver, size_t max_iter_line_search) {
        qn_oracle o{};
        o.kind = QN_ORACLE_OBJECTIVE;
        o.memoize = 1;
        o.objective = objective.handle();
        return make_result(qn_minimize(h_, &line_search.ffi(), &o, max_iter_solver, max_iter_line_search, nullptr, nullptr));
    }
    template <class LS>
    Result minimize(LS& line_search, const Multinomial& objective, size_t max_iter_solver, size_t max_iter_line_search) {
        qn_oracle o{};
        o.kind = QN_ORACLE_OBJECTIVE;
        o.memoize = 1;
        o.objective = objective.handle();
        return make_result(qn_minimize(h_, &line_search.ffi(), &o, max_iter_solver, max_iter_line_search, nullptr, nullptr));
    }
    template <class LS>
    Result minimize(LS& line_search, const SparseMultinomial& objective, size_t max_iter_solver, size_t max_iter_line_search) {
        qn_oracle o{};
        o.kind = QN_ORACLE_OBJECTIVE;
        o.memoize = 1;
        o.objective = objective.handle();
        return make_result(qn_minimize(h_, &line_search.ffi(), &o, max_iter_solver, max_iter_line_search, nullptr, nullptr));
    }
    template <class LS>
    Result minimize(LS& line_search, const SparseLogistic& objective, size_t max_iter_solver, size_t max_iter_line_search) {
        qn_oracle o{};
        o.kind = QN_ORACLE_OBJECTIVE;
        o.memoize = 1;
        o.objective = objective.handle();
        return make_result(qn_minimize(h_, &line_search.ffi(), &o, max_iter_solver, max_iter_line_search, nullptr, nullptr));
    }
    template <class LS>
    Result minimize(LS& line_search, const SparseQuadratic& objective, size_t max_iter_solver, size_t max_iter_line_search) {
        qn_oracle o{};
        o.kind = QN_ORACLE_OBJECTIVE;
        o.memoize = 1;
        o.objective = objective.handle();
        return make_result(qn_minimize(h_, &line_search.ffi(), &o, max_iter_solver, max_iter_line_search, nullptr, nullptr));
    }
};

using BFGS = LineSearchSolver<QN_BFGS>;                       // quasi_newton/bfgs.rs
using DFP = LineSearchSolver<QN_DFP>;                         // quasi_newton/dfp.rs
using GradientDescent = LineSearchSolver<QN_GRADIENT_DESCENT>; // steepest_descent/gradient_descent.rs
using Broyden = LineSearchSolver<QN_BROYDEN>;                 // quasi_newton/broyden.rs
// newton/mod.rs: d = -H^-1 g.  The closure returns FuncEvalMultivariate(f, g).with_hessian(h), or the oracle is a device objective: a Quadratic
// (its own matrix) or a LogSumExp (the Hessian formed on the device at every x_k).
using Newton = LineSearchSolver<QN_NEWTON>;

using CoordinateDescent = LineSearchSolver<QN_COORDINATE_DESCENT>; // steepest_descent/coordinate_descent.rs: d = -e_p, p the first index of the largest |g_i|

// steepest_descent/pnorm_descent.rs: new(grad_tol, x0, inverse_p) with inverse_p column-major n x n (DMatrix); d = (-inverse_p) * g
class PnormDescent : public LineSearchSolver<QN_PNORM_DESCENT> {
  public:
    PnormDescent(Floating grad_tol, const DVector& x0, const DVector& inverse_p_colmajor, Context& ctx = Context::default_context())
        : LineSearchSolver<QN_PNORM_DESCENT>(grad_tol, x0, ctx) {
        if (inverse_p_colmajor.size() != x0.size() * x0.size()) throw SolverError(QN_ERROR_INPUT_PARAMS);
        check(qn_solver_set_inverse_p(this->handle(), inverse_p_colmajor.data()));
    }
    static PnormDescent new_(Floating grad_tol, const DVector& x0, const DVector& inverse_p_colmajor) { return PnormDescent(grad_tol, x0, inverse_p_colmajor); }
    Floating grad_tol() const { return this->tol(); }
    DVector inverse_p() const { const size_t n = this->x().size(); DVector m(n * n); check(qn_solver_get_inverse_p(this->handle(), m.data())); return m; }
};

// quasi_newton/broyden_b.rs: new(tol, x0, lower_bound, upper_bound); x0 is projected (:51), d = P(x - H g) - x (:73-77); everything else is Broyden's
class BroydenB : public LineSearchSolver<QN_BROYDEN> {
    DVector lb_, ub_;
  public:
    BroydenB(Floating tol, const DVector& x0, DVector lower_bound, DVector upper_bound, Context& ctx = Context::default_context())
        : LineSearchSolver<QN_BROYDEN>(tol, x0, ctx), lb_(std::move(lower_bound)), ub_(std::move(upper_bound)) {
        check(qn_solver_set_bounds(this->handle(), lb_.data(), ub_.data()));
    }
    static BroydenB new_(Floating tol, const DVector& x0, DVector lb, DVector ub) { return BroydenB(tol, x0, std::move(lb), std::move(ub)); }
    const DVector& lower_bound() const { return lb_; }
    const DVector& upper_bound() const { return ub_; }
};

// The bounded first-order solvers (O(n) device memory): the box, projected_gradient (ls_solver.rs:121-133), has_converged on its
// infinity norm (spg.rs:89-92, projected_gradient_descent.rs:76-83).
template <int METHOD>
class ProjectedSolver : public LineSearchSolver<METHOD> {
    DVector lb_, ub_;
  public:
    ProjectedSolver(Floating grad_tol, const DVector& x0, DVector lower_bound, DVector upper_bound, Context& ctx = Context::default_context())
        : LineSearchSolver<METHOD>(grad_tol, x0, ctx), lb_(std::move(lower_bound)), ub_(std::move(upper_bound)) {
        check(qn_solver_set_bounds(this->handle(), lb_.data(), ub_.data())); // x0.box_projection(..), spg.rs:35
    }
    Floating grad_tol() const { return this->tol(); }
    const DVector& lower_bound() const { return lb_; }
    const DVector& upper_bound() const { return ub_; }
    DVector projected_gradient(const FuncEvalMultivariate& eval) const {
        DVector pg = eval.g();
        const DVector& x = this->x();
        for (size_t i = 0; i < pg.size(); ++i)
            if ((x[i] == lb_[i] && pg[i] > 0.0) || (x[i] == ub_[i] && pg[i] < 0.0)) pg[i] = 0.0;
        return pg;
    }
    bool has_converged(const FuncEvalMultivariate& eval) const {
        Floating acc = -INFINITY;
        for (Floating v : projected_gradient(eval)) acc = std::fmax(std::fabs(v), acc);
        return acc < this->tol();
    }
    DVector compute_direction(const FuncEvalMultivariate& eval) const { // spg.rs:76-86 / projected_gradient_descent.rs:51-60
        DVector d(eval.g().size());
        check(qn_solver_compute_direction(this->handle(), eval.g().data(), d.data()));
        return d;
    }
};

// steepest_descent/projected_gradient_descent.rs: new(grad_tol, x0, lower_bound, upper_bound)
class ProjectedGradientDescent : public ProjectedSolver<QN_PROJECTED_GRADIENT> {
  public:
    using ProjectedSolver<QN_PROJECTED_GRADIENT>::ProjectedSolver;
    static ProjectedGradientDescent new_(Floating grad_tol, const DVector& x0, DVector lb, DVector ub) {
        return ProjectedGradientDescent(grad_tol, x0, std::move(lb), std::move(ub));
    }
};

// steepest_descent/spg.rs: new(grad_tol, x0, &mut oracle, lower_bound, upper_bound) -- the constructor calls the oracle for lambda0 (:40-46)
class SpectralProjectedGradient : public ProjectedSolver<QN_SPG> {
  public:
    template <class Oracle>
    SpectralProjectedGradient(Floating grad_tol, const DVector& x0, Oracle&& oracle, DVector lower_bound, DVector upper_bound,
                              Context& ctx = Context::default_context())
        : ProjectedSolver<QN_SPG>(grad_tol, x0, std::move(lower_bound), std::move(upper_bound), ctx) {
        GLLQuadratic ls(1e-4, 1);
        Result r = this->minimize(ls, oracle, 0, 0); // no iteration: the constructor's evaluation only
        if (r.is_err() && r.unwrap_err().kind != SolverError::MaxIterReached) r.unwrap();
    }
    template <class Oracle>
    static SpectralProjectedGradient new_(Floating grad_tol, const DVector& x0, Oracle&& oracle, DVector lb, DVector ub) {
        return SpectralProjectedGradient(grad_tol, x0, oracle, std::move(lb), std::move(ub));
    }
    SpectralProjectedGradient with_lambdas(Floating lambda_min, Floating lambda_max) && { // spg.rs:23-27
        check(qn_solver_set_spg_lambdas(this->handle(), lambda_min, lambda_max));
        return std::move(*this);
    }
    Floating lambda() const { Floating v = 0; int some = 0; check(qn_solver_spg_lambda(this->handle(), &v, &some)); return v; }
};

// Spectral proximal gradient (SpaRSA): min f(x) + sum_j l1_j |x_j| over lb <= x <= ub -- SpectralProjectedGradient with the projection replaced by the
// proximal map of lambda l1 |.| plus the box, GLLQuadratic or BackTracking on the composite value.  new_(tol, x0, oracle, l1) with one scalar or n
// entries, with_bounds(lb, ub) before the first minimize; the constructor calls the oracle once, for lambda0.  Entries the prox sets to zero are 0.0.
class SpectralProximalGradient : public LineSearchSolver<QN_SPECTRAL_PROXIMAL_GRADIENT> {
    using Base = LineSearchSolver<QN_SPECTRAL_PROXIMAL_GRADIENT>;
    DVector lb_, ub_;
    template <class Oracle>
    void lambda0(Oracle&& oracle) {
        GLLQuadratic ls(1e-4, 1);
        Result r = this->minimize(ls, oracle, 0, 0); // no iteration: the constructor's evaluation only
        if (r.is_err() && r.unwrap_err().kind != SolverError::MaxIterReached) r.unwrap();
    }
  public:
    template <class Oracle>
    SpectralProximalGradient(Floating tol, const DVector& x0, Oracle&& oracle, const DVector& l1, Context& ctx = Context::default_context()) : Base(tol, x0, ctx) {
        set_l1(l1);
        lambda0(oracle);
    }
    template <class Oracle>
    SpectralProximalGradient(Floating tol, const DVector& x0, Oracle&& oracle, Floating l1, Context& ctx = Context::default_context()) : Base(tol, x0, ctx) {
        set_l1(l1);
        lambda0(oracle);
    }
    template <class Oracle>
    SpectralProximalGradient(Floating tol, const DVector& x0, Oracle&& oracle, const DVector& l1, DVector lower_bound, DVector upper_bound,
                             Context& ctx = Context::default_context())
        : Base(tol, x0, ctx), lb_(std::move(lower_bound)), ub_(std::move(upper_bound)) {
        check(qn_solver_set_bounds(this->handle(), lb_.data(), ub_.data()));
        set_l1(l1);
        lambda0(oracle);
    }
    template <class Oracle, class L1>
    static SpectralProximalGradient new_(Floating tol, const DVector& x0, Oracle&& oracle, const L1& l1) { return SpectralProximalGradient(tol, x0, oracle, l1); }
    template <class Oracle>
    static SpectralProximalGradient new_(Floating tol, const DVector& x0, Oracle&& oracle, const DVector& l1, DVector lb, DVector ub) {
        return SpectralProximalGradient(tol, x0, oracle, l1, std::move(lb), std::move(ub));
    }
    // between two minimize calls: GLLQuadratic's ring is cleared; lambda, x and the memoised evaluation of the smooth part are kept
    void set_l1(const DVector& l1) {
        if (l1.size() != this->x().size()) throw SolverError(QN_ERROR_INPUT_PARAMS);
        check(qn_solver_set_l1(this->handle(), l1.data(), 0.0));
    }
    void set_l1(Floating l1) { check(qn_solver_set_l1(this->handle(), nullptr, l1)); }
    DVector l1() const { DVector v(this->x().size()); check(qn_solver_get_l1(this->handle(), v.data())); return v; }
    SpectralProximalGradient with_lambdas(Floating lambda_min, Floating lambda_max) && {
        check(qn_solver_set_spg_lambdas(this->handle(), lambda_min, lambda_max));
        return std::move(*this);
    }
    Floating lambda() const { Floating v = 0; int some = 0; check(qn_solver_spg_lambda(this->handle(), &v, &some)); return v; }
    Floating grad_tol() const { return this->tol(); }
    Floating penalty() const { // h at x()
        const DVector w = l1();
        const DVector& x = this->x();
        Floating h = 0.0;
        for (size_t i = 0; i < x.size(); ++i) h += w[i] * std::fabs(x[i]);
        return h;
    }
    Floating composite(const FuncEvalMultivariate& eval) const { return eval.f() + penalty(); }
    size_t nonzeros() const { size_t c = 0; for (Floating v : this->x()) c += v != 0.0; return c; }
    // per entry the element of least magnitude of the subdifferential of f + h at x(), opened towards the side a bound blocks; its infinity norm
    Floating measure(const FuncEvalMultivariate& eval) const {
        const DVector w = l1();
        const DVector& x = this->x();
        Floating acc = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            const Floating g = eval.g()[i];
            Floating lo = x[i] > 0.0 ? g + w[i] : g - w[i], hi = x[i] < 0.0 ? g - w[i] : g + w[i];
            if (!lb_.empty() && x[i] == lb_[i]) lo = -INFINITY;
            if (!ub_.empty() && x[i] == ub_[i]) hi = INFINITY;
            acc = std::fmax(acc, std::fabs(lo > 0.0 ? lo : (hi < 0.0 ? hi : 0.0)));
        }
        return acc;
    }
    bool has_converged(const FuncEvalMultivariate& eval) const { return measure(eval) < this->tol(); }
};

// newton/projected_newton.rs: new(grad_tol, x0, lower_bound, upper_bound); d = P(x - H^-1 g) - x, H^-1 g by one Cholesky factorisation (the
// Hessian's lower triangle) and one solve on the GPU.  The closure returns FuncEvalMultivariate(f, g).with_hessian(h), or the oracle is a Quadratic.
class ProjectedNewton : public ProjectedSolver<QN_PROJECTED_NEWTON> {
  public:
    using ProjectedSolver<QN_PROJECTED_NEWTON>::ProjectedSolver;
    static ProjectedNewton new_(Floating grad_tol, const DVector& x0, DVector lb, DVector ub) {
        return ProjectedNewton(grad_tol, x0, std::move(lb), std::move(ub));
    }
    bool has_converged(const FuncEvalMultivariate& eval) const { // projected_newton.rs:95-110
        if (this->next_iterate_too_close() || this->gradient_next_iterate_too_close()) return true;
        return ProjectedSolver<QN_PROJECTED_NEWTON>::has_converged(eval);
    }
    size_t newton_factorisations() const { size_t v = 0; check(qn_solver_newton_factorisations(this->handle(), &v)); return v; }
};

// newton/spn.rs: new(grad_tol, x0, &mut oracle, lower_bound, upper_bound); d = P(x - lambda H^-1 g) - x, lambda as in SpectralProjectedGradient
class SpectralProjectedNewton : public ProjectedSolver<QN_SPECTRAL_PROJECTED_NEWTON> {
  public:
    template <class Oracle>
    SpectralProjectedNewton(Floating grad_tol, const DVector& x0, Oracle&& oracle, DVector lower_bound, DVector upper_bound,
                            Context& ctx = Context::default_context())
        : ProjectedSolver<QN_SPECTRAL_PROJECTED_NEWTON>(grad_tol, x0, std::move(lower_bound), std::move(upper_bound), ctx) {
        GLLQuadratic ls(1e-4, 1);
        Result r = this->minimize(ls, oracle, 0, 0); // no iteration: the constructor's evaluation only (spn.rs:40-46)
        if (r.is_err() && r.unwrap_err().kind != SolverError::MaxIterReached) r.unwrap();
    }
    template <class Oracle>
    static SpectralProjectedNewton new_(Floating grad_tol, const DVector& x0, Oracle&& oracle, DVector lb, DVector ub) {
        return SpectralProjectedNewton(grad_tol, x0, oracle, std::move(lb), std::move(ub));
    }
    SpectralProjectedNewton with_lambdas(Floating lambda_min, Floating lambda_max) && { // spn.rs:23-27
        check(qn_solver_set_spg_lambdas(this->handle(), lambda_min, lambda_max));
        return std::move(*this);
    }
    Floating lambda() const { Floating v = 0; int some = 0; check(qn_solver_spg_lambda(this->handle(), &v, &some)); return v; }
    size_t newton_factorisations() const { size_t v = 0; check(qn_solver_newton_factorisations(this->handle(), &v)); return v; }
};

// Limited-memory BFGS in a box: new(tol, x0, lower_bound, upper_bound).with_memory(m); d = P(x - H_k g) - x, H_k g from the last m pairs (s, y) by the
// compact form (two streams of the memory and one small solve per iteration on the GPU).  NOT the reference's Fortran-backed Lbfgsb: no generalised
// Cauchy point, no subspace minimisation -- the bounded variant follows BFGSB's convention (bfgs_b.rs:72-75).
class ProjectedLBFGS : public ProjectedSolver<QN_LBFGS> {
  public:
    using ProjectedSolver<QN_LBFGS>::ProjectedSolver;
    static ProjectedLBFGS new_(Floating tol, const DVector& x0, DVector lb, DVector ub) { return ProjectedLBFGS(tol, x0, std::move(lb), std::move(ub)); }
    ProjectedLBFGS with_memory(size_t m) && { check(qn_solver_set_lbfgs_memory(this->handle(), m)); return std::move(*this); }
    size_t memory() const { size_t v = 0; check(qn_solver_lbfgs_state(this->handle(), &v, nullptr, nullptr, nullptr)); return v; }
    size_t stored_pairs() const { size_t v = 0; check(qn_solver_lbfgs_state(this->handle(), nullptr, &v, nullptr, nullptr)); return v; }
    Floating gamma() const { Floating v = 0; check(qn_solver_lbfgs_state(this->handle(), nullptr, nullptr, &v, nullptr)); return v; }
    size_t resets() const { size_t v = 0; check(qn_solver_lbfgs_state(this->handle(), nullptr, nullptr, nullptr, &v)); return v; }
};

// Limited-memory BFGS: new(tol, x0).with_memory(m); d = -H_k g.  The same solver with the box left at (-inf, +inf).
class LBFGS : public ProjectedLBFGS {
  public:
    LBFGS(Floating tol, const DVector& x0, Context& ctx = Context::default_context())
        : ProjectedLBFGS(tol, x0, DVector(x0.size(), -INFINITY), DVector(x0.size(), INFINITY), ctx) {}
    static LBFGS new_(Floating tol, const DVector& x0) { return LBFGS(tol, x0); }
    LBFGS with_memory(size_t m) && { check(qn_solver_set_lbfgs_memory(this->handle(), m)); return std::move(*this); }
};

// Orthant-wise limited-memory quasi-Newton (OWL-QN, Andrew and Gao 2007): min f(x) + sum_j l1_j |x_j|, UNBOUNDED ONLY.  new_(tol, x0, l1) with one
// scalar or n entries, .with_memory(m); LBFGS's memory and direction kernels applied to the pseudo-gradient, the direction aligned with it, every trial
// point projected onto the orthant of x; BackTracking only, on the composite value.  Entries the projection switches off are exactly 0.0.  The pairs
// are differences of the smooth gradient: set_l1 between two minimize calls keeps them, x and the memoised evaluation (the regularisation path).
class OWLQN : public LineSearchSolver<QN_OWLQN> {
    using Base = LineSearchSolver<QN_OWLQN>;
  public:
    OWLQN(Floating tol, const DVector& x0, const DVector& l1, Context& ctx = Context::default_context()) : Base(tol, x0, ctx) { set_l1(l1); }
    OWLQN(Floating tol, const DVector& x0, Floating l1, Context& ctx = Context::default_context()) : Base(tol, x0, ctx) { set_l1(l1); }
    template <class L1>
    static OWLQN new_(Floating tol, const DVector& x0, const L1& l1) { return OWLQN(tol, x0, l1); }
    OWLQN with_memory(size_t m) && { check(qn_solver_set_lbfgs_memory(this->handle(), m)); return std::move(*this); }
    void set_memory(size_t m) { check(qn_solver_set_lbfgs_memory(this->handle(), m)); } // the stored pairs are dropped
    void set_l1(const DVector& l1) {
        if (l1.size() != this->x().size()) throw SolverError(QN_ERROR_INPUT_PARAMS);
        check(qn_solver_set_l1(this->handle(), l1.data(), 0.0));
    }
    void set_l1(Floating l1) { check(qn_solver_set_l1(this->handle(), nullptr, l1)); }
    DVector l1() const { DVector v(this->x().size()); check(qn_solver_get_l1(this->handle(), v.data())); return v; }
    size_t memory() const { size_t v = 0; check(qn_solver_lbfgs_state(this->handle(), &v, nullptr, nullptr, nullptr)); return v; }
    size_t stored_pairs() const { size_t v = 0; check(qn_solver_lbfgs_state(this->handle(), nullptr, &v, nullptr, nullptr)); return v; }
    Floating gamma() const { Floating v = 0; check(qn_solver_lbfgs_state(this->handle(), nullptr, nullptr, &v, nullptr)); return v; }
    size_t resets() const { size_t v = 0; check(qn_solver_lbfgs_state(this->handle(), nullptr, nullptr, nullptr, &v)); return v; }
    Floating grad_tol() const { return this->tol(); }
    // v of the last loop top
    DVector pseudo_gradient() const { DVector v(this->x().size()); check(qn_solver_get_pseudo_gradient(this->handle(), v.data())); return v; }
    Floating penalty() const { // h at x()
        const DVector w = l1();
        const DVector& x = this->x();
        Floating h = 0.0;
        for (size_t i = 0; i < x.size(); ++i) h += w[i] * std::fabs(x[i]);
        return h;
    }
    Floating composite(const FuncEvalMultivariate& eval) const { return eval.f() + penalty(); }
    size_t nonzeros() const { size_t c = 0; for (Floating v : this->x()) c += v != 0.0; return c; }
    // the infinity norm of the pseudo-gradient at x() from an evaluation of the smooth part there: SpectralProximalGradient's measure without a box
    Floating measure(const FuncEvalMultivariate& eval) const {
        const DVector w = l1();
        const DVector& x = this->x();
        Floating acc = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            const Floating g = eval.g()[i];
            const Floating lo = x[i] > 0.0 ? g + w[i] : g - w[i], hi = x[i] < 0.0 ? g - w[i] : g + w[i];
            acc = std::fmax(acc, std::fabs(lo > 0.0 ? lo : (hi < 0.0 ? hi : 0.0)));
        }
        return acc;
    }
    bool has_converged(const FuncEvalMultivariate& eval) const { return measure(eval) < this->tol(); }
};

// Nonlinear conjugate gradient: new(tol, x0).with_variant(NonlinearCG::Variant::HZ, powell_nu, restart_every); d+ = beta d - g+, one extra vector of
// state on the GPU.  Restarts d = -g by Powell's test |g+.g| >= powell_nu g+.g+ (INFINITY: off), every restart_every iterations (0: never) and whenever
// beta d - g+ would not descend.  UNBOUNDED ONLY; StrongWolfe (what FR, DY and HS+ assume) or BackTracking.  has_converged: ||g||_inf < tol.
class NonlinearCG : public LineSearchSolver<QN_NONLINEAR_CG> {
  public:
    enum class Variant : int { FR = QN_CG_FR, PR_PLUS = QN_CG_PR_PLUS, HS_PLUS = QN_CG_HS_PLUS, DY = QN_CG_DY, HZ = QN_CG_HZ };
    using LineSearchSolver<QN_NONLINEAR_CG>::LineSearchSolver;
    static NonlinearCG new_(Floating tol, const DVector& x0) { return NonlinearCG(tol, x0); }
    NonlinearCG with_variant(Variant v, Floating powell_nu = 0.2, size_t restart_every = 0) && {
        check(qn_solver_set_cg(this->handle(), static_cast<int>(v), powell_nu, restart_every)); // (the stored direction is dropped)
        return std::move(*this);
    }
    Variant variant() const { int v = 0; check(qn_solver_cg_state(this->handle(), &v, nullptr, nullptr, nullptr)); return static_cast<Variant>(v); }
    Floating beta() const { Floating v = 0; check(qn_solver_cg_state(this->handle(), nullptr, &v, nullptr, nullptr)); return v; }
    size_t restarts() const { size_t v = 0; check(qn_solver_cg_state(this->handle(), nullptr, nullptr, &v, nullptr)); return v; }
    size_t since_restart() const { size_t v = 0; check(qn_solver_cg_state(this->handle(), nullptr, nullptr, nullptr, &v)); return v; }
};

// Truncated Newton: new(tol, x0).with_inner(eta_max, max_inner, chunk); Newton's direction from a few conjugate-gradient steps on H z = g, each
// costing one Hessian-vector product of the device LogSumExp or Logistic objective (one stream of A, never a matrix).  UNBOUNDED ONLY; those two only
// (n_pad <= 16384); BackTracking or StrongWolfe, first trial t = 1.  has_converged: ||g||_inf < tol.
class NewtonCG : public LineSearchSolver<QN_NEWTON_CG> {
  public:
    using LineSearchSolver<QN_NEWTON_CG>::LineSearchSolver;
    static NewtonCG new_(Floating tol, const DVector& x0) { return NewtonCG(tol, x0); }
    NewtonCG with_inner(Floating eta_max = 0.5, size_t max_inner = 0, size_t chunk = 8) && {
        check(qn_solver_set_newton_cg(this->handle(), eta_max, max_inner, chunk));
        return std::move(*this);
    }
    // the inner loop's preconditioner: QN_PRECOND_NONE (the default) or QN_PRECOND_JACOBI, the diagonal of H(x_k) by one more pass of A per outer
    // iteration.  It pays where the columns of A differ in scale by orders of magnitude; on well-scaled columns, or with m < n and a small mu, it buys
    // nothing or loses.  LogSumExp, Logistic and SparseLogistic only (another objective: ErrorInputParams at minimize)
    void set_preconditioner(int kind) { check(qn_solver_set_newton_cg_preconditioner(this->handle(), kind)); }
    int preconditioner() const { int v = 0; check(qn_solver_newton_cg_precond_state(this->handle(), &v, nullptr, nullptr)); return v; }
    size_t diag_passes() const { size_t v = 0; check(qn_solver_newton_cg_precond_state(this->handle(), nullptr, &v, nullptr)); return v; }
    size_t diag_floored() const { size_t v = 0; check(qn_solver_newton_cg_precond_state(this->handle(), nullptr, nullptr, &v)); return v; }
    size_t inner_last() const { size_t v = 0; check(qn_solver_newton_cg_state(this->handle(), &v, nullptr, nullptr, nullptr, nullptr)); return v; }
    size_t inner_total() const { size_t v = 0; check(qn_solver_newton_cg_state(this->handle(), nullptr, &v, nullptr, nullptr, nullptr)); return v; }
    size_t hv_passes() const { size_t v = 0; check(qn_solver_newton_cg_state(this->handle(), nullptr, nullptr, &v, nullptr, nullptr)); return v; }
    size_t negative_curvature() const { size_t v = 0; check(qn_solver_newton_cg_state(this->handle(), nullptr, nullptr, nullptr, &v, nullptr)); return v; }
    size_t fallbacks() const { size_t v = 0; check(qn_solver_newton_cg_state(this->handle(), nullptr, nullptr, nullptr, nullptr, &v)); return v; }
};

} // namespace optimization_solvers
