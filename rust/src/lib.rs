//! The solver traits of `optimization-solvers` (src/ls_solver.rs:3-112, src/line_search/mod.rs:14-23) implemented on
//! libqn_hip.so -- hand-written gfx950 kernels behind the C ABI of include/qn_hip.h.
//!
//! NOT COMPILED in the build image (no Rust toolchain; see ../Cargo.toml).  The FFI declarations are checked against the
//! header mechanically; every call sequence below is exercised on the GPU from Python (tests/test_gpu_trait_hooks.py,
//! tests/test_gpu_parity.py) and C (examples/ffi_consumer.c).
//!
//! Two ways in, both with the reference's names and signatures:
//!
//! * **the whole loop on the device** -- `GpuBFGS::minimize_on_device(&mut ls, oracle, max_iter_solver, max_iter_line_search,
//!   callback)` has the argument list of `LineSearchSolver::minimize` (ls_solver.rs:66-111) and takes a GPU line search.  One
//!   `qn_minimize` call runs every iteration; the closure is called through a trampoline in exactly the reference's order.
//!   `minimize_objective` takes a device-resident objective instead (no host round trip at all: the benchmark path).
//!   (It is NOT called `minimize`: an inherent method of that name would shadow the trait's for every call site, including
//!   those that pass the reference's own `MoreThuente` / `BackTracking`, which are not GPU line searches -- a compile error
//!   where a fall-back was meant.  `solver.minimize(..)` therefore always means the trait method below.)
//! * **hook by hook** -- `impl ComputeDirection` / `impl LineSearchSolver` provide `compute_direction`, `has_converged`,
//!   `update_next_iterate`, `xk`, `k`, ... so generic code written against the traits (`fn run<S: LineSearchSolver>(..)`)
//!   drives the reference's own template loop with the matrix work (H g, the secant update) on the GPU, and
//!   `impl LineSearch for GpuMoreThuente / GpuBackTracking` runs the line search's state machine on the GPU.
pub mod ffi;

use ffi::*;
use nalgebra::{DMatrix, DVector};
use optimization_solvers::{
    ComputeDirection, CurvatureCondition, Floating, FuncEvalMultivariate, HasBounds, LineSearch, LineSearchSolver, MoreThuente,
    SolverError, SufficientDecreaseCondition,
};
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::sync::OnceLock;

// ------------------------------------------------------------------------------------------------
// status <-> SolverError (ls_solver.rs:10-20)
// ------------------------------------------------------------------------------------------------
fn status_to_result(code: c_int) -> Result<(), SolverError> {
    match code {
        QN_OK => Ok(()),
        QN_MAX_ITER_REACHED => Err(SolverError::MaxIterReached),
        QN_OUT_OF_DOMAIN => Err(SolverError::OutOfDomain),
        QN_ERROR_INPUT_PARAMS => Err(SolverError::ErrorInputParams),
        _ => Err(SolverError::AbnormalTermination),
    }
}

/// Thread-local detail of the last non-OK return.
pub fn last_error() -> String {
    unsafe { CStr::from_ptr(qn_last_error_message()).to_string_lossy().into_owned() }
}

// ------------------------------------------------------------------------------------------------
// context: one GPU, one stream.  There is no CPU fallback: without a usable MI355X this panics.
// ------------------------------------------------------------------------------------------------
struct CtxPtr(*mut qn_context);
unsafe impl Send for CtxPtr {}
unsafe impl Sync for CtxPtr {}
static DEFAULT_CTX: OnceLock<CtxPtr> = OnceLock::new();

/// The process-wide context on device 0 (created on first use, never destroyed).
pub fn default_context() -> *mut qn_context {
    DEFAULT_CTX
        .get_or_init(|| {
            let mut ctx = std::ptr::null_mut();
            let code = unsafe { qn_context_create(0, &mut ctx) };
            assert_eq!(code, QN_OK, "qn_context_create: {} (there is no CPU fallback)", last_error());
            CtxPtr(ctx)
        })
        .0
}

// ------------------------------------------------------------------------------------------------
// the oracle closure `impl FnMut(&DVector<Floating>) -> FuncEvalMultivariate` behind a `void* user`
// ------------------------------------------------------------------------------------------------
unsafe extern "C" fn oracle_trampoline<F>(user: *mut c_void, x: *const f64, n: usize, f: *mut f64, g: *mut f64) -> c_int
where
    F: FnMut(&DVector<Floating>) -> FuncEvalMultivariate,
{
    let oracle = &mut *(user as *mut F);
    let xv = DVector::from_column_slice(std::slice::from_raw_parts(x, n));
    let eval = oracle(&xv);
    if eval.g().len() != n {
        return 1; // aborts the run with QN_ABNORMAL_TERMINATION
    }
    *f = *eval.f();
    std::ptr::copy_nonoverlapping(eval.g().as_ptr(), g, n);
    0
}

/// The Hessian part of the closure's `FuncEvalMultivariate` (func_eval.rs:8,27-33), column-major as `DMatrix` stores it: asked for by
/// the projected Newton solvers only.  A closure without one ends the run ("Hessian not available in the oracle").
unsafe extern "C" fn hessian_trampoline<F>(user: *mut c_void, x: *const f64, n: usize, h: *mut f64) -> c_int
where
    F: FnMut(&DVector<Floating>) -> FuncEvalMultivariate,
{
    let oracle = &mut *(user as *mut F);
    let xv = DVector::from_column_slice(std::slice::from_raw_parts(x, n));
    let eval = oracle(&xv);
    match eval.hessian() {
        Some(m) if m.nrows() == n && m.ncols() == n => {
            std::ptr::copy_nonoverlapping(m.as_ptr(), h, n * n);
            0
        }
        _ => 1,
    }
}

fn host_oracle<F>(oracle: &mut F, memoize: bool, with_hessian: bool) -> qn_oracle
where
    F: FnMut(&DVector<Floating>) -> FuncEvalMultivariate,
{
    qn_oracle {
        kind: QN_ORACLE_HOST,
        memoize: memoize as i32, // 0: the reference's call sequence, call for call
        host_fn: Some(oracle_trampoline::<F>),
        host_user: oracle as *mut F as *mut c_void,
        device_fn: None,
        device_user: std::ptr::null_mut(),
        objective: std::ptr::null_mut(),
        // only the projected Newton solvers ask for the Hessian: every other solver passes the oracle it always passed
        host_hessian_fn: if with_hessian { Some(hessian_trampoline::<F>) } else { None },
    }
}

// ------------------------------------------------------------------------------------------------
// line searches
// ------------------------------------------------------------------------------------------------
/// A line search the device state machine knows: hands its parameters over as the plain `qn_linesearch` struct.
pub trait GpuLineSearch: LineSearch {
    fn ffi(&mut self) -> &mut qn_linesearch;
}

/// `MoreThuente` (morethuente.rs:6-62) with the state machine of `compute_step_len` (:165-297) on the GPU.
#[derive(Clone, Debug)]
pub struct GpuMoreThuente {
    ls: qn_linesearch,
}

impl Default for GpuMoreThuente {
    fn default() -> Self {
        let mut ls = unsafe { std::mem::zeroed::<qn_linesearch>() };
        unsafe { qn_morethuente_default(&mut ls) }; // c1 1e-4, c2 0.9, t in [0, inf), deltas 0.58333333 / 0.66 / 1.1
        GpuMoreThuente { ls }
    }
}

impl From<&MoreThuente> for GpuMoreThuente {
    /// Same parameters as a reference line search (its fields are readable through derive_getters).
    fn from(m: &MoreThuente) -> Self {
        let mut out = GpuMoreThuente::default();
        out.ls.c1 = *m.c1();
        out.ls.c2 = *m.c2();
        out.ls.t_min = *m.t_min();
        out.ls.t_max = *m.t_max();
        out.ls.delta_min = *m.delta_min();
        out.ls.delta = *m.delta();
        out.ls.delta_max = *m.delta_max();
        out
    }
}

impl GpuMoreThuente {
    // the builder methods of morethuente.rs:31-62; the reference's assert!s stay panics
    pub fn with_deltas(mut self, delta_min: Floating, delta: Floating, delta_max: Floating) -> Self {
        assert_eq!(unsafe { qn_morethuente_with_deltas(&mut self.ls, delta_min, delta, delta_max) }, QN_OK, "{}", last_error());
        self
    }
    pub fn with_t_min(mut self, t_min: Floating) -> Self {
        assert_eq!(unsafe { qn_morethuente_with_t_min(&mut self.ls, t_min) }, QN_OK, "{}", last_error());
        self
    }
    pub fn with_t_max(mut self, t_max: Floating) -> Self {
        assert_eq!(unsafe { qn_morethuente_with_t_max(&mut self.ls, t_max) }, QN_OK, "{}", last_error());
        self
    }
    pub fn with_c1(mut self, c1: Floating) -> Self {
        assert_eq!(unsafe { qn_morethuente_with_c1(&mut self.ls, c1) }, QN_OK, "{}", last_error());
        self
    }
    pub fn with_c2(mut self, c2: Floating) -> Self {
        assert_eq!(unsafe { qn_morethuente_with_c2(&mut self.ls, c2) }, QN_OK, "{}", last_error());
        self
    }
}

/// `BackTracking` (backtracking.rs:3-58).  The reference keeps `beta` private without a getter, so this is constructed
/// from the same two numbers rather than converted from a `BackTracking`.
#[derive(Clone, Debug)]
pub struct GpuBackTracking {
    ls: qn_linesearch,
}

impl GpuBackTracking {
    pub fn new(c1: Floating, beta: Floating) -> Self {
        let mut ls = unsafe { std::mem::zeroed::<qn_linesearch>() };
        unsafe { qn_backtracking_new(&mut ls, c1, beta) };
        GpuBackTracking { ls }
    }
}

fn step_len_on_device<F>(
    ls: &mut qn_linesearch,
    x_k: &DVector<Floating>,
    eval_x_k: &FuncEvalMultivariate,
    direction_k: &DVector<Floating>,
    oracle: &mut F,
    max_iter: usize,
) -> Floating
where
    F: FnMut(&DVector<Floating>) -> FuncEvalMultivariate,
{
    let o = host_oracle(oracle, false, false);
    let mut t = 0.0;
    let code = unsafe {
        qn_compute_step_len(
            default_context(),
            ls,
            x_k.as_ptr(),
            *eval_x_k.f(),
            eval_x_k.g().as_ptr(),
            direction_k.as_ptr(),
            x_k.len(),
            &o,
            max_iter,
            &mut t,
        )
    };
    // the trait returns a bare Floating (line_search/mod.rs:22): a HIP failure can only panic
    assert_eq!(code, QN_OK, "qn_compute_step_len: {}", last_error());
    t
}

macro_rules! impl_line_search {
    ($t:ty) => {
        impl LineSearch for $t {
            fn compute_step_len(
                &mut self,
                x_k: &DVector<Floating>,
                eval_x_k: &FuncEvalMultivariate,
                direction_k: &DVector<Floating>,
                oracle: &mut impl FnMut(&DVector<Floating>) -> FuncEvalMultivariate,
                max_iter: usize,
            ) -> Floating {
                step_len_on_device(&mut self.ls, x_k, eval_x_k, direction_k, oracle, max_iter)
            }
        }
        impl GpuLineSearch for $t {
            fn ffi(&mut self) -> &mut qn_linesearch {
                &mut self.ls
            }
        }
    };
}
impl_line_search!(GpuMoreThuente);
impl_line_search!(GpuBackTracking);

/// `GLLQuadratic` (gll_quadratic.rs): the reference keeps its fields private without getters, so this is constructed from the
/// same numbers.  The history `f_previous` is kept by the SOLVER on the device (qn_hip.h), not by this value.
#[derive(Clone, Debug)]
pub struct GpuGLLQuadratic {
    ls: qn_linesearch,
}

impl GpuGLLQuadratic {
    pub fn new(c1: Floating, m: usize) -> Self {
        let mut ls = unsafe { std::mem::zeroed::<qn_linesearch>() };
        unsafe { qn_gll_quadratic_new(&mut ls, c1, m) };
        GpuGLLQuadratic { ls }
    }
    pub fn with_sigmas(mut self, sigma1: Floating, sigma2: Floating) -> Self {
        unsafe { qn_gll_quadratic_with_sigmas(&mut self.ls, sigma1, sigma2) };
        self
    }
}
impl_line_search!(GpuGLLQuadratic);

/// The strong-Wolfe search of the O(n) solvers (QN_LS_STRONG_WOLFE): MINPACK-2 `dcsrch`, one oracle call per trial; no counterpart among the
/// reference's line searches.  `c1` = ftol, `c2` = gtol (0 < c1 < c2 < 1, checked by `minimize`); xtol 0.1, t_min 0, t_max 1e10.  With bounds of
/// its own every search is clipped to the box; `t_max` is never modified.  The trait's `compute_step_len` on its own is not built for this kind
/// (it panics with the library's message): use it through `minimize`.
#[derive(Clone, Debug)]
pub struct GpuStrongWolfe {
    ls: qn_linesearch,
    lb: Option<DVector<Floating>>,
    ub: Option<DVector<Floating>>,
}

impl GpuStrongWolfe {
    pub fn new(c1: Floating, c2: Floating) -> Self {
        let mut ls = unsafe { std::mem::zeroed::<qn_linesearch>() };
        unsafe { qn_strong_wolfe_new(&mut ls, c1, c2) };
        GpuStrongWolfe { ls, lb: None, ub: None }
    }
    pub fn with_xtol(mut self, xtol: Floating) -> Self {
        assert_eq!(unsafe { qn_strong_wolfe_with_xtol(&mut self.ls, xtol) }, QN_OK, "{}", last_error());
        self
    }
    pub fn with_t_min(mut self, t_min: Floating) -> Self {
        assert_eq!(unsafe { qn_morethuente_with_t_min(&mut self.ls, t_min) }, QN_OK, "{}", last_error());
        self
    }
    pub fn with_t_max(mut self, t_max: Floating) -> Self {
        assert_eq!(unsafe { qn_morethuente_with_t_max(&mut self.ls, t_max) }, QN_OK, "{}", last_error());
        self
    }
    pub fn with_lower_bound(mut self, lb: DVector<Floating>) -> Self {
        self.lb = Some(lb);
        self
    }
    pub fn with_upper_bound(mut self, ub: DVector<Floating>) -> Self {
        self.ub = Some(ub);
        self
    }
    /// the bounds live in this value: their addresses are bound right before every call (a moved value keeps no stale pointer)
    fn bind(&mut self) -> &mut qn_linesearch {
        if let Some(lb) = &self.lb {
            unsafe { qn_linesearch_with_lower_bound(&mut self.ls, lb.as_ptr()) };
        }
        if let Some(ub) = &self.ub {
            unsafe { qn_linesearch_with_upper_bound(&mut self.ls, ub.as_ptr()) };
        }
        &mut self.ls
    }
}
impl Default for GpuStrongWolfe {
    fn default() -> Self {
        Self::new(1e-4, 0.9)
    }
}
impl LineSearch for GpuStrongWolfe {
    fn compute_step_len(
        &mut self,
        x_k: &DVector<Floating>,
        eval_x_k: &FuncEvalMultivariate,
        direction_k: &DVector<Floating>,
        oracle: &mut impl FnMut(&DVector<Floating>) -> FuncEvalMultivariate,
        max_iter: usize,
    ) -> Floating {
        step_len_on_device(self.bind(), x_k, eval_x_k, direction_k, oracle, max_iter)
    }
}
impl GpuLineSearch for GpuStrongWolfe {
    fn ffi(&mut self) -> &mut qn_linesearch {
        self.bind()
    }
}
impl SufficientDecreaseCondition for GpuStrongWolfe {
    fn c1(&self) -> Floating {
        self.ls.c1
    }
}
impl CurvatureCondition for GpuStrongWolfe {
    fn c2(&self) -> Floating {
        self.ls.c2
    }
}

/// The exact step `t = -g.d / d'Qd` on a device quadratic (QN_LS_EXACT_QUADRATIC; `DeviceObjective::quadratic` / `sparse_quadratic`, driven by
/// `minimize_objective`) for `GpuSpectralProjectedGradient`, `GpuProjectedGradientDescent`, `GpuLBFGS` and `GpuNonlinearCG` -- with the last, linear
/// conjugate gradients.  One product `Q d` per iteration; no value of f is compared.  `refresh_every` = 1: the objective evaluates every accepted
/// point; k > 1: every k-th; 0: never (the gradient follows `g + t Q d`), except that convergence is only declared on a gradient the objective
/// evaluated.  A closure has no `Q`: the trait's `compute_step_len` and `minimize` with a closure fail with the library's message.
#[derive(Clone, Debug)]
pub struct GpuExactQuadratic {
    ls: qn_linesearch,
}

impl GpuExactQuadratic {
    pub fn new(refresh_every: usize) -> Self {
        let mut ls = unsafe { std::mem::zeroed::<qn_linesearch>() };
        unsafe { qn_exact_quadratic_new(&mut ls, refresh_every.min(i32::MAX as usize) as c_int) };
        GpuExactQuadratic { ls }
    }
    pub fn refresh_every(&self) -> usize {
        self.ls._pad as usize
    }
}
impl Default for GpuExactQuadratic {
    fn default() -> Self {
        Self::new(1)
    }
}
impl_line_search!(GpuExactQuadratic);

/// `NoSearch` (nosearch.rs): `compute_step_len` returns 1.0 and never calls the oracle.  On the device it pairs with
/// `GpuGradientDescent`, `GpuCoordinateDescent`, `GpuPnormDescent` (and Newton): the solvers on the trait's default update hook.
#[derive(Clone, Debug)]
pub struct GpuNoSearch {
    ls: qn_linesearch,
}

impl GpuNoSearch {
    pub fn new() -> Self {
        let mut ls = unsafe { std::mem::zeroed::<qn_linesearch>() };
        unsafe { qn_nosearch_new(&mut ls) };
        GpuNoSearch { ls }
    }
}
impl Default for GpuNoSearch {
    fn default() -> Self {
        Self::new()
    }
}
impl_line_search!(GpuNoSearch);
impl SufficientDecreaseCondition for GpuGLLQuadratic {
    fn c1(&self) -> Floating {
        self.ls.c1
    }
}

// The condition traits of line_search/mod.rs:25-83, as the reference implements them for its own structs (morethuente.rs,
// backtracking.rs:13-18): only the sensitivities are supplied, the tests themselves are the traits' default methods (and
// `WolfeConditions` follows from the blanket impl, mod.rs:85-86).
impl SufficientDecreaseCondition for GpuMoreThuente {
    fn c1(&self) -> Floating {
        self.ls.c1
    }
}
impl CurvatureCondition for GpuMoreThuente {
    fn c2(&self) -> Floating {
        self.ls.c2
    }
}
impl SufficientDecreaseCondition for GpuBackTracking {
    fn c1(&self) -> Floating {
        self.ls.bt_c1
    }
}

// ------------------------------------------------------------------------------------------------
// a device-resident objective (the benchmark's dense quadratic; log-sum-exp): evaluated by the library's own kernels
// ------------------------------------------------------------------------------------------------
pub struct DeviceObjective {
    h: *mut qn_objective,
    n: usize,
}

impl DeviceObjective {
    /// f = 1/2 x'Qx - b'x, g = Qx - b; `q_rowmajor` is the full symmetric n x n matrix.
    pub fn quadratic(q_rowmajor: &[Floating], b: &DVector<Floating>) -> Result<Self, SolverError> {
        let n = b.len();
        if q_rowmajor.len() != n * n {
            return Err(SolverError::ErrorInputParams);
        }
        let mut h = std::ptr::null_mut();
        status_to_result(unsafe { qn_quadratic_create(default_context(), n, q_rowmajor.as_ptr(), b.as_ptr(), &mut h) })?;
        Ok(DeviceObjective { h, n })
    }
    /// f = log sum_i exp(a_i'x + c_i) + mu/2 ||x||^2; `a_rowmajor` is m x n.
    pub fn log_sum_exp(a_rowmajor: &[Floating], c: &DVector<Floating>, n: usize, mu: Floating) -> Result<Self, SolverError> {
        let m = c.len();
        if a_rowmajor.len() != m * n {
            return Err(SolverError::ErrorInputParams);
        }
        let mut h = std::ptr::null_mut();
        status_to_result(unsafe { qn_logsumexp_create(default_context(), m, n, a_rowmajor.as_ptr(), c.as_ptr(), mu, &mut h) })?;
        Ok(DeviceObjective { h, n })
    }
    /// f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2; `a_rowmajor` is m x n, `y` holds -1 / +1 exactly (0 / 1 labels: pass 2 y - 1),
    /// `weights` (>= 0, a 0 masks its row) defaults to ones.  The objective of GpuLBFGS, GpuNonlinearCG, the spectral family and GpuNewtonCG.
    pub fn logistic(a_rowmajor: &[Floating], y: &DVector<Floating>, weights: Option<&DVector<Floating>>, n: usize, mu: Floating) -> Result<Self, SolverError> {
        let m = y.len();
        if a_rowmajor.len() != m * n || weights.map_or(false, |w| w.len() != m) {
            return Err(SolverError::ErrorInputParams);
        }
        let mut h = std::ptr::null_mut();
        let w = weights.map_or(std::ptr::null(), |w| w.as_ptr());
        status_to_result(unsafe { qn_logistic_create(default_context(), m, n, a_rowmajor.as_ptr(), y.as_ptr(), w, mu, &mut h) })?;
        Ok(DeviceObjective { h, n })
    }
    /// The logistic objective with a sparse A in CSR (m x n; `indptr` has m + 1 entries, the columns of a row increase strictly) and no limit on
    /// n: the device keeps A and A' (24 bytes per nonzero), so the transpose product needs no atomics.  Labels, weights and mu as `logistic`.
    pub fn sparse_logistic(indptr: &[i64], indices: &[i64], data: &[Floating], y: &DVector<Floating>, weights: Option<&DVector<Floating>>, n: usize,
                           mu: Floating) -> Result<Self, SolverError> {
        let m = y.len();
        if indptr.len() != m + 1 || indices.len() != data.len() || weights.map_or(false, |w| w.len() != m) {
            return Err(SolverError::ErrorInputParams);
        }
        let (no_index, no_value) = ([0i64; 1], [0.0; 1]); // an empty matrix: the library takes a dangling pointer for what it is
        let ci = if indices.is_empty() { no_index.as_ptr() } else { indices.as_ptr() };
        let va = if data.is_empty() { no_value.as_ptr() } else { data.as_ptr() };
        let w = weights.map_or(std::ptr::null(), |w| w.as_ptr());
        let mut h = std::ptr::null_mut();
        status_to_result(unsafe {
            qn_sparse_logistic_create(default_context(), m, n, data.len(), indptr.as_ptr() as *const c_void, ci as *const c_void, 8, va, y.as_ptr(), w, mu, &mut h)
        })?;
        Ok(DeviceObjective { h, n })
    }
    /// Softmax regression, class-major: x[k n + j] = W[k, j], N = n_classes * n entries.  `a_rowmajor` is m x n, `labels` holds m classes in
    /// 0 .. n_classes, `weights` (>= 0, a 0 masks its row) defaults to ones.  The objective of GpuLBFGS, GpuNonlinearCG, the spectral family and GpuNewtonCG.
    pub fn multinomial(a_rowmajor: &[Floating], labels: &[i32], n_classes: usize, weights: Option<&DVector<Floating>>, n: usize, mu: Floating) -> Result<Self, SolverError> {
        let m = labels.len();
        if a_rowmajor.len() != m * n || weights.map_or(false, |w| w.len() != m) {
            return Err(SolverError::ErrorInputParams);
        }
        let mut h = std::ptr::null_mut();
        let w = weights.map_or(std::ptr::null(), |w| w.as_ptr());
        status_to_result(unsafe { qn_multinomial_create(default_context(), m, n, n_classes, a_rowmajor.as_ptr(), labels.as_ptr() as *const c_void, w, mu, &mut h) })?;
        Ok(DeviceObjective { h, n: n * n_classes })
    }
    /// Softmax regression with a sparse A in CSR (m x n; `indptr` has m + 1 entries, the columns of a row increase strictly), class-major as
    /// `multinomial`: N = n_classes * n entries, with no limit on N.  The device keeps A and A' (24 bytes per nonzero) and feature-major copies of
    /// the class-major vectors: no atomics, every sum in one fixed order.  Labels, weights and mu as `multinomial`.
    pub fn sparse_multinomial(indptr: &[i64], indices: &[i64], data: &[Floating], labels: &[i32], n_classes: usize, weights: Option<&DVector<Floating>>,
                              n: usize, mu: Floating) -> Result<Self, SolverError> {
        let m = labels.len();
        if indptr.len() != m + 1 || indices.len() != data.len() || weights.map_or(false, |w| w.len() != m) {
            return Err(SolverError::ErrorInputParams);
        }
        let (no_index, no_value) = ([0i64; 1], [0.0; 1]); // an empty matrix: the library takes a dangling pointer for what it is
        let ci = if indices.is_empty() { no_index.as_ptr() } else { indices.as_ptr() };
        let va = if data.is_empty() { no_value.as_ptr() } else { data.as_ptr() };
        let w = weights.map_or(std::ptr::null(), |w| w.as_ptr());
        let mut h = std::ptr::null_mut();
        status_to_result(unsafe {
            qn_sparse_multinomial_create(default_context(), m, n, n_classes, data.len(), indptr.as_ptr() as *const c_void, ci as *const c_void, 8, va,
                                         labels.as_ptr() as *const c_void, w, mu, &mut h)
        })?;
        Ok(DeviceObjective { h, n: n * n_classes })
    }
    /// f = 1/2 x'Qx - b'x with a sparse Q in CSR (both triangles of a symmetric matrix; `indptr` has n + 1 entries, the columns of a row
    /// increase strictly): the large objective of the O(n) solvers (GpuSpectralProjectedGradient, GpuProjectedGradientDescent, GpuLBFGS).
    pub fn sparse_quadratic(indptr: &[i64], indices: &[i64], data: &[Floating], b: &DVector<Floating>) -> Result<Self, SolverError> {
        let n = b.len();
        if indptr.len() != n + 1 || indices.len() != data.len() {
            return Err(SolverError::ErrorInputParams);
        }
        let (no_index, no_value) = ([0i64; 1], [0.0; 1]); // an empty matrix: the library takes a dangling pointer for what it is
        let ci = if indices.is_empty() { no_index.as_ptr() } else { indices.as_ptr() };
        let va = if data.is_empty() { no_value.as_ptr() } else { data.as_ptr() };
        let mut h = std::ptr::null_mut();
        status_to_result(unsafe {
            qn_sparse_quadratic_create(default_context(), n, data.len(), indptr.as_ptr() as *const c_void, ci as *const c_void, 8, va, b.as_ptr(), &mut h)
        })?;
        Ok(DeviceObjective { h, n })
    }
    /// A sparse quadratic's shape: (nnz, lanes per row in use, rows summed by a workgroup of their own, Q == Q' bit for bit).
    pub fn sparse_info(&self) -> Result<(usize, i32, usize, bool), SolverError> {
        let (mut nnz, mut lanes, mut long_rows, mut sym) = (0usize, 0 as c_int, 0usize, 0 as c_int);
        status_to_result(unsafe { qn_objective_sparse_info(self.h, &mut nnz, &mut lanes, &mut long_rows, &mut sym) })?;
        Ok((nnz, lanes as i32, long_rows, sym != 0))
    }
    /// Lanes that share one row of a sparse quadratic: 1, 2, 4, .. 64; 0: chosen from the mean row length.
    pub fn set_lanes_per_row(&mut self, lanes: i32) -> Result<(), SolverError> {
        status_to_result(unsafe { qn_sparse_quadratic_set_lanes_per_row(self.h, lanes as c_int) })
    }
    /// One evaluation at a host point (`let eval = f_and_g(&x)` after `minimize`).
    pub fn eval(&self, x: &DVector<Floating>) -> Result<FuncEvalMultivariate, SolverError> {
        if x.len() != self.n {
            return Err(SolverError::ErrorInputParams);
        }
        let mut f = 0.0;
        let mut g = DVector::zeros(self.n);
        status_to_result(unsafe { qn_objective_eval(self.h, x.as_ptr(), &mut f, g.as_mut_ptr()) })?;
        Ok(FuncEvalMultivariate::new(f, g))
    }
    /// The Hessian at a host point (`FuncEvalMultivariate::hessian()` after `minimize`): Q for a quadratic, for log-sum-exp the matrix
    /// the device kernel forms for `GpuNewton` (A'(diag(p) - p p')A + mu I, symmetric bit for bit).
    pub fn hessian(&self, x: &DVector<Floating>) -> Result<DMatrix<Floating>, SolverError> {
        if x.len() != self.n {
            return Err(SolverError::ErrorInputParams);
        }
        let mut m = DMatrix::<Floating>::zeros(self.n, self.n);
        status_to_result(unsafe { qn_objective_hessian(self.h, x.as_ptr(), m.as_mut_ptr()) })?; // column-major, like DMatrix
        Ok(m)
    }
    /// (Q v, v'Qv) of a dense or a sparse quadratic: one pass over the matrix and no evaluation of f -- what the exact step
    /// `-g.d / d'Qd` along d costs, and what a conjugate-gradient loop of the caller's own needs.  Log-sum-exp: `ErrorInputParams`.
    pub fn hess_vec(&self, v: &DVector<Floating>) -> Result<(DVector<Floating>, Floating), SolverError> {
        if v.len() != self.n {
            return Err(SolverError::ErrorInputParams);
        }
        let mut c = 0.0;
        let mut q = DVector::zeros(self.n);
        status_to_result(unsafe { qn_objective_hess_vec(self.h, v.as_ptr(), q.as_mut_ptr(), &mut c) })?;
        Ok((q, c))
    }
    /// (H(x) v, v'H(x)v) without the matrix.  Log-sum-exp: the softmax weights at x, then one stream of A for
    /// A'(p o (A v)) - gbar (p . (A v)) + mu v (n_pad <= 16384, one rank; otherwise `ErrorInputParams`).  A quadratic: x is not read,
    /// the call is `hess_vec(v)` bit for bit.
    pub fn hess_vec_at(&self, x: &DVector<Floating>, v: &DVector<Floating>) -> Result<(DVector<Floating>, Floating), SolverError> {
        if x.len() != self.n || v.len() != self.n {
            return Err(SolverError::ErrorInputParams);
        }
        let mut c = 0.0;
        let mut q = DVector::zeros(self.n);
        status_to_result(unsafe { qn_objective_hess_vec_at(self.h, x.as_ptr(), v.as_ptr(), q.as_mut_ptr(), &mut c) })?;
        Ok((q, c))
    }
    /// diag H(x) without the matrix: the weights at x, then one pass over A with squared entries.  Log-sum-exp, logistic (n_pad <= 16384,
    /// one rank) and sparse logistic; every other objective: `ErrorInputParams` (not built).
    pub fn hess_diag_at(&self, x: &DVector<Floating>) -> Result<DVector<Floating>, SolverError> {
        if x.len() != self.n {
            return Err(SolverError::ErrorInputParams);
        }
        let mut d = DVector::zeros(self.n);
        status_to_result(unsafe { qn_objective_hess_diag_at(self.h, x.as_ptr(), d.as_mut_ptr()) })?;
        Ok(d)
    }
}

impl Drop for DeviceObjective {
    fn drop(&mut self) {
        unsafe { qn_objective_destroy(self.h) }
    }
}

// ------------------------------------------------------------------------------------------------
// solvers
// ------------------------------------------------------------------------------------------------
/// What GpuBFGS / GpuDFP / GpuGradientDescent share: the device handle and the host mirror of (x, k) that `xk()` / `k()`
/// hand out by reference (ls_solver.rs:24-27).
struct Core {
    h: *mut qn_solver,
    n: usize,
    tol: Floating,
    x: DVector<Floating>,
    k: usize,
    // the box of the bounded first-order solvers (spg.rs:15-16); (-inf, +inf) for every other solver
    lb: DVector<Floating>,
    ub: DVector<Floating>,
}

impl Core {
    fn new(method: c_int, tol: Floating, x0: DVector<Floating>) -> Self {
        let mut h = std::ptr::null_mut();
        let code = unsafe { qn_solver_create(default_context(), method, tol, x0.as_ptr(), x0.len(), &mut h) };
        assert_eq!(code, QN_OK, "qn_solver_create: {}", last_error());
        let n = x0.len();
        Core { h, n, tol, x: x0, k: 0, lb: DVector::from_element(n, Floating::NEG_INFINITY), ub: DVector::from_element(n, Floating::INFINITY) }
    }
    /// `qn_solver_set_bounds`: stores the box, projects x on the device (spg.rs:35) and mirrors the projected x
    fn set_bounds(&mut self, lb: DVector<Floating>, ub: DVector<Floating>) -> Result<(), SolverError> {
        if lb.len() != self.n || ub.len() != self.n {
            return Err(SolverError::ErrorInputParams);
        }
        status_to_result(unsafe { qn_solver_set_x(self.h, self.x.as_ptr()) })?;
        status_to_result(unsafe { qn_solver_set_bounds(self.h, lb.as_ptr(), ub.as_ptr()) })?;
        self.lb = lb;
        self.ub = ub;
        unsafe { qn_solver_get_x(self.h, self.x.as_mut_ptr()) };
        Ok(())
    }
    /// ls_solver.rs:121-133 with the exact comparisons; the gradient itself where the box is infinite
    fn projected_gradient(&self, eval: &FuncEvalMultivariate) -> DVector<Floating> {
        let mut pg = eval.g().clone();
        for (i, x) in self.x.iter().enumerate() {
            if (x == &self.lb[i] && pg[i] > 0.0) || (x == &self.ub[i] && pg[i] < 0.0) {
                pg[i] = 0.0;
            }
        }
        pg
    }
    fn option(&self, f: unsafe extern "C" fn(*mut qn_solver, *mut f64, *mut c_int) -> c_int) -> Option<Floating> {
        let (mut v, mut some) = (0.0, 0);
        unsafe { f(self.h, &mut v, &mut some) };
        if some != 0 {
            Some(v)
        } else {
            None
        }
    }
    fn flag(&self, f: unsafe extern "C" fn(*mut qn_solver, *mut c_int) -> c_int) -> bool {
        let mut v = 0;
        unsafe { f(self.h, &mut v) };
        v != 0
    }
    /// host mirror -> device (the caller may have written through `xk_mut()` / `k_mut()`)
    fn push(&mut self) -> Result<(), SolverError> {
        status_to_result(unsafe { qn_solver_set_x(self.h, self.x.as_ptr()) })?;
        status_to_result(unsafe { qn_solver_set_k(self.h, self.k) })
    }
    /// device -> host mirror
    fn pull(&mut self) {
        unsafe {
            qn_solver_get_x(self.h, self.x.as_mut_ptr());
            self.k = qn_solver_k(self.h);
        }
    }
    fn approx_inv_hessian(&self) -> DMatrix<Floating> {
        let mut m = DMatrix::zeros(self.n, self.n);
        let code = unsafe { qn_solver_get_inv_hessian(self.h, m.as_mut_ptr(), 1) }; // column-major, like DMatrix
        assert_eq!(code, QN_OK, "qn_solver_get_inv_hessian: {}", last_error());
        m
    }
    fn direction(&mut self, eval: &FuncEvalMultivariate) -> Result<DVector<Floating>, SolverError> {
        if eval.g().len() != self.n {
            return Err(SolverError::ErrorInputParams);
        }
        let mut d = DVector::zeros(self.n);
        status_to_result(unsafe { qn_solver_compute_direction(self.h, eval.g().as_ptr(), d.as_mut_ptr()) })?;
        Ok(d)
    }
    fn minimize_with(&mut self, ls: &mut qn_linesearch, o: &qn_oracle, max_iter_solver: usize, max_iter_line_search: usize,
                     callback: qn_callback_fn, callback_user: *mut c_void) -> Result<(), SolverError> {
        self.push()?;
        let code = unsafe { qn_minimize(self.h, ls, o, max_iter_solver, max_iter_line_search, callback, callback_user) };
        self.pull();
        status_to_result(code)
    }
}

impl Drop for Core {
    fn drop(&mut self) {
        unsafe { qn_solver_destroy(self.h) }
    }
}

macro_rules! gpu_solver {
    ($(#[$doc:meta])* $name:ident, $method:expr, $quasi_newton:expr) => {
        $(#[$doc])*
        pub struct $name {
            core: Core,
        }

        impl $name {
            pub fn new(tol: Floating, x0: DVector<Floating>) -> Self {
                $name { core: Core::new($method, tol, x0) }
            }
            // the getters derive_getters generates on the reference struct (bfgs.rs:3-12)
            pub fn x(&self) -> &DVector<Floating> {
                &self.core.x
            }
            pub fn tol(&self) -> &Floating {
                &self.core.tol
            }

            /// `LineSearchSolver::minimize` (ls_solver.rs:66-111), the whole loop in ONE `qn_minimize` call.  Same argument
            /// list as the trait method, but under ANOTHER NAME on purpose: Rust resolves `solver.minimize(..)` to an
            /// inherent method of that name before it looks at traits, so an inherent `minimize<LS: GpuLineSearch>` would have
            /// turned every call site that passes one of the reference's own line searches (`MoreThuente`, `BackTracking`:
            /// not `GpuLineSearch`) into a compile error instead of a fall-back.  As it is, `solver.minimize(..)` is the
            /// trait's default method for ANY `LS: LineSearch` (hook by hook through the ABI, see `impl LineSearchSolver`
            /// below), and `solver.minimize_on_device(..)` is the fast path for the GPU line searches.  The closure is
            /// called in exactly the reference's order: loop top (:79), every line-search evaluation, the gradient at the
            /// accepted point (bfgs.rs:98).
            pub fn minimize_on_device<LS: GpuLineSearch>(
                &mut self,
                line_search: &mut LS,
                mut oracle: impl FnMut(&DVector<Floating>) -> FuncEvalMultivariate,
                max_iter_solver: usize,
                max_iter_line_search: usize,
                mut callback: Option<&mut dyn FnMut(&Self)>,
            ) -> Result<(), SolverError> {
                struct CallbackEnv<'a, 'b> {
                    me: *mut $name,
                    f: &'a mut Option<&'b mut dyn FnMut(&$name)>,
                }
                unsafe extern "C" fn callback_trampoline(user: *mut c_void, _solver: *mut qn_solver) {
                    let env = &mut *(user as *mut CallbackEnv);
                    (*env.me).core.pull(); // the callback sees the state after `k += 1` (ls_solver.rs:104-107)
                    if let Some(f) = env.f.as_mut() {
                        f(&*env.me)
                    }
                }
                let o = host_oracle(&mut oracle, false, $method == QN_NEWTON || $method == QN_PROJECTED_NEWTON || $method == QN_SPECTRAL_PROJECTED_NEWTON);
                let has_callback = callback.is_some();
                let mut env = CallbackEnv { me: self as *mut $name, f: &mut callback };
                let core = &mut self.core as *mut Core; // (`env.me` aliases self for the duration of the call)
                unsafe {
                    (*core).minimize_with(
                        line_search.ffi(),
                        &o,
                        max_iter_solver,
                        max_iter_line_search,
                        if has_callback { Some(callback_trampoline) } else { None },
                        &mut env as *mut CallbackEnv as *mut c_void,
                    )
                }
            }

            /// The benchmark path: a device-resident objective, nothing crosses PCIe per iteration.  Each DISTINCT point is
            /// evaluated once (`qn_oracle.memoize = 1`): the values fed to the algorithm are those of the reference's call
            /// sequence, only the number of evaluations differs (5 -> 2 per iteration for More-Thuente on a quadratic).
            pub fn minimize_objective<LS: GpuLineSearch>(
                &mut self,
                line_search: &mut LS,
                objective: &DeviceObjective,
                max_iter_solver: usize,
                max_iter_line_search: usize,
            ) -> Result<(), SolverError> {
                if objective.n != self.core.n {
                    return Err(SolverError::ErrorInputParams);
                }
                let o = qn_oracle {
                    kind: QN_ORACLE_OBJECTIVE,
                    memoize: 1,
                    host_fn: None,
                    host_user: std::ptr::null_mut(),
                    device_fn: None,
                    device_user: std::ptr::null_mut(),
                    objective: objective.h,
                    host_hessian_fn: None,
                };
                self.core.minimize_with(line_search.ffi(), &o, max_iter_solver, max_iter_line_search, None, std::ptr::null_mut())
            }
        }

        impl ComputeDirection for $name {
            /// bfgs.rs:42-49 / dfp.rs:42-49 (`-H g`, one pass over the device-resident matrix); gradient_descent.rs:24-30 (`-g`)
            fn compute_direction(&mut self, eval_x_k: &FuncEvalMultivariate) -> Result<DVector<Floating>, SolverError> {
                self.core.direction(eval_x_k)
            }
        }

        impl LineSearchSolver for $name {
            fn xk(&self) -> &DVector<Floating> {
                &self.core.x
            }
            fn xk_mut(&mut self) -> &mut DVector<Floating> {
                &mut self.core.x
            }
            fn k(&self) -> &usize {
                &self.core.k
            }
            fn k_mut(&mut self) -> &mut usize {
                &mut self.core.k
            }
            fn has_converged(&self, eval: &FuncEvalMultivariate) -> bool {
                if $quasi_newton {
                    // bfgs.rs:64-76
                    self.core.flag(qn_solver_next_iterate_too_close)
                        || self.core.flag(qn_solver_gradient_next_iterate_too_close)
                        || eval.g().norm() < self.core.tol
                } else {
                    // gradient_descent.rs:46-53: infinity norm; spg.rs:89-92, projected_gradient_descent.rs:76-83: of the projected
                    // gradient (the gradient itself while the box is infinite, as for GradientDescent)
                    self.core.projected_gradient(eval).iter().fold(Floating::NEG_INFINITY, |acc, x| x.abs().max(acc)) < self.core.tol
                }
            }

            /// The hook of bfgs.rs:78-130 / dfp.rs:78-118: line search, next iterate, s and y on the host (n-vectors), the
            /// secant update of the n x n matrix on the device.  With a `GpuMoreThuente` / `GpuBackTracking` the line
            /// search's state machine runs on the GPU as well.
            fn update_next_iterate<LS: LineSearch>(
                &mut self,
                line_search: &mut LS,
                eval_x_k: &FuncEvalMultivariate,
                oracle: &mut impl FnMut(&DVector<Floating>) -> FuncEvalMultivariate,
                direction: &DVector<Floating>,
                max_iter_line_search: usize,
            ) -> Result<(), SolverError> {
                if $method == QN_PROJECTED_NEWTON || $method == QN_SPECTRAL_PROJECTED_NEWTON {
                    // the direction needs the Cholesky solve and (spn.rs) the device-resident lambda: `minimize_on_device` / `minimize_objective`
                    return Err(SolverError::ErrorInputParams);
                }
                if $method == QN_OWLQN {
                    // the accepted point is the trial kernel's orthant projection, never x + t d, and the pairs live on the device: `minimize_on_device` / `minimize_objective`
                    return Err(SolverError::ErrorInputParams);
                }
                if $method == QN_SPG || $method == QN_SPECTRAL_PROXIMAL_GRADIENT {
                    // spg.rs:126-143 updates lambda here; it lives on the device and only qn_minimize updates it.  Refuse rather than run
                    // a fixed-lambda projected gradient under SPG's name: use `minimize_on_device` / `minimize_objective`.
                    return Err(SolverError::ErrorInputParams);
                }
                let step = line_search.compute_step_len(self.xk(), eval_x_k, direction, oracle, max_iter_line_search);
                let next_iterate = self.xk() + step * direction;
                if $quasi_newton {
                    let s = &next_iterate - self.xk();
                    let y = oracle(&next_iterate).g() - eval_x_k.g();
                    *self.xk_mut() = next_iterate;
                    status_to_result(unsafe { qn_solver_set_x(self.core.h, self.core.x.as_ptr()) })?;
                    // s_norm / y_norm, the two "too close" early returns and the update itself (bfgs.rs:96-127)
                    status_to_result(unsafe { qn_solver_secant_update(self.core.h, s.as_ptr(), y.as_ptr()) })
                } else {
                    *self.xk_mut() = next_iterate; // ls_solver.rs:60-62
                    Ok(())
                }
            }
        }
    };
}

gpu_solver!(
    /// Drop-in for `BFGS` (quasi_newton/bfgs.rs:4-130): the dense inverse Hessian lives in HBM and never leaves it.
    GpuBFGS, QN_BFGS, true
);
gpu_solver!(
    /// Drop-in for `DFP` (quasi_newton/dfp.rs).
    GpuDFP, QN_DFP, true
);
gpu_solver!(
    /// Drop-in for `Broyden` (quasi_newton/broyden.rs): H += ((s - H y) s') H / (s . y) as written.  The inverse Hessian is not symmetric after
    /// the first update; the GPU streams it whole, once per iteration (QN_PATH_RANK1).
    GpuBroyden, QN_BROYDEN, true
);
gpu_solver!(
    /// Drop-in for `BroydenB` (quasi_newton/broyden_b.rs): `new(tol, x0).with_bounds(lb, ub)` stands for `new(tol, x0, lb, ub)`;
    /// x0 is projected, d = P(x - H g) - x.
    GpuBroydenB, QN_BROYDEN, true
);
gpu_solver!(
    /// Drop-in for `GradientDescent` (steepest_descent/gradient_descent.rs:7-82); `tol` is its `grad_tol`.
    GpuGradientDescent, QN_GRADIENT_DESCENT, false
);

gpu_solver!(
    /// Drop-in for `Newton` (newton/mod.rs:8-69): d = -H^-1 g from a blocked Cholesky on the f64 matrix cores (a pivoted LU when the Hessian is not
    /// positive definite).  The closure's `FuncEvalMultivariate` carries the Hessian (`with_hessian`), or the oracle is a device objective
    /// (`minimize_objective`): a quadratic's own matrix, or the log-sum-exp Hessian formed on the device at every x_k.
    GpuNewton, QN_NEWTON, false
);
gpu_solver!(
    /// Drop-in for `CoordinateDescent` (steepest_descent/coordinate_descent.rs), as written: d = -e_p with p the first index of the largest
    /// |g_i| -- whatever the sign of g_p (`-max_value.signum()` of a magnitude, coordinate_descent.rs:43).  `tol` is its `grad_tol`.
    GpuCoordinateDescent, QN_COORDINATE_DESCENT, false
);
gpu_solver!(
    /// Drop-in for `PnormDescent` (steepest_descent/pnorm_descent.rs): `new(grad_tol, x0).with_inverse_p(&inverse_p)` stands for
    /// `new(grad_tol, x0, inverse_p)`; d = (-inverse_p) * g, one read-only stream of the matrix per iteration on the GPU (QN_PATH_PNORM).
    GpuPnormDescent, QN_PNORM_DESCENT, false
);
impl GpuPnormDescent {
    /// The constructor's third argument (pnorm_descent.rs:20): any n x n matrix, kept by the solver for its whole life.
    pub fn with_inverse_p(self, inverse_p: &DMatrix<Floating>) -> Self {
        assert_eq!((inverse_p.nrows(), inverse_p.ncols()), (self.core.n, self.core.n), "inverse_p must be n x n");
        let code = unsafe { qn_solver_set_inverse_p(self.core.h, inverse_p.as_ptr()) }; // column-major, like DMatrix
        assert_eq!(code, QN_OK, "qn_solver_set_inverse_p: {}", last_error());
        self
    }
    /// `inverse_p()` of derive_getters (pnorm_descent.rs:11-17), downloaded.
    pub fn inverse_p(&self) -> DMatrix<Floating> {
        let mut m = DMatrix::<Floating>::zeros(self.core.n, self.core.n);
        let code = unsafe { qn_solver_get_inverse_p(self.core.h, m.as_mut_ptr()) };
        assert_eq!(code, QN_OK, "qn_solver_get_inverse_p: {}", last_error());
        m
    }
    pub fn grad_tol(&self) -> &Floating {
        &self.core.tol
    }
}
impl GpuCoordinateDescent {
    pub fn grad_tol(&self) -> &Floating {
        &self.core.tol
    }
}

gpu_solver!(
    /// Drop-in for `ProjectedGradientDescent` (steepest_descent/projected_gradient_descent.rs): `new(grad_tol, x0).with_bounds(lb, ub)`
    /// stands for `new(grad_tol, x0, lb, ub)`.  O(n) device memory, the device-wide vector kernels (QN_PATH_VECTOR).
    GpuProjectedGradientDescent, QN_PROJECTED_GRADIENT, false
);
gpu_solver!(
    /// Drop-in for `SpectralProjectedGradient` (steepest_descent/spg.rs).  `new(grad_tol, x0).with_bounds(lb, ub)`; the
    /// constructor's oracle call (spg.rs:40-46, lambda0) is made by the first `minimize_on_device` / `minimize_objective`.
    /// The Barzilai-Borwein scalar lives on the device and is updated by `qn_minimize` only: drive this solver with
    /// `minimize_on_device`, not hook by hook through the trait's default `minimize`: its `update_next_iterate` returns
    /// `ErrorInputParams` (and `compute_direction` does before the first device call has formed lambda0).
    GpuSpectralProjectedGradient, QN_SPG, false
);

gpu_solver!(
    /// Drop-in for `ProjectedNewton` (newton/projected_newton.rs): `new(grad_tol, x0).with_bounds(lb, ub)`; d = P(x - H^-1 g) - x from one
    /// Cholesky factorisation (the Hessian's lower triangle) and one solve on the GPU (QN_PATH_PNEWTON).  The closure's `FuncEvalMultivariate`
    /// carries the Hessian (`with_hessian`), or the oracle is a device quadratic.  Drive it with `minimize_on_device` / `minimize_objective`.
    GpuProjectedNewton, QN_PROJECTED_NEWTON, false
);
gpu_solver!(
    /// Drop-in for `SpectralProjectedNewton` (newton/spn.rs): d = P(x - lambda H^-1 g) - x, lambda as in `GpuSpectralProjectedGradient`.
    GpuSpectralProjectedNewton, QN_SPECTRAL_PROJECTED_NEWTON, false
);

gpu_solver!(
    /// Limited-memory BFGS in a box: `new(tol, x0).with_bounds(lb, ub).with_memory(m)`; d = P(x - H_k g) - x with H_k g from the last m pairs
    /// (s, y) in the compact form -- two streams of the memory and one small solve per iteration on the GPU (QN_PATH_LBFGS).  NOT the reference's
    /// `Lbfgsb` (the Fortran L-BFGS-B: no generalised Cauchy point, no subspace minimisation here); the bounded variant follows `BFGSB`'s
    /// convention (bfgs_b.rs:72-75).  Drive it with `minimize_on_device` / `minimize_objective`: the memory lives on the device.
    GpuProjectedLbfgs, QN_LBFGS, false
);
gpu_solver!(
    /// Limited-memory BFGS: `new(tol, x0).with_memory(m)`; d = -H_k g.  `GpuProjectedLbfgs` with the box left at (-inf, +inf).
    GpuLbfgs, QN_LBFGS, false
);

macro_rules! lbfgs_memory {
    ($name:ident) => {
        impl $name {
            /// 1 <= m <= 32 (default 5, as `Lbfgsb::new`, lbfgsb.rs:91); the stored pairs are dropped
            pub fn with_memory(self, m: usize) -> Self {
                assert_eq!(unsafe { qn_solver_set_lbfgs_memory(self.core.h, m) }, QN_OK, "{}", last_error());
                self
            }
            /// (m, pairs stored, gamma of the last direction, times the safeguard g.z > 0 cleared the memory)
            pub fn lbfgs_state(&self) -> (usize, usize, Floating, usize) {
                let (mut m, mut stored, mut gamma, mut resets) = (0usize, 0usize, 0.0, 0usize);
                assert_eq!(unsafe { qn_solver_lbfgs_state(self.core.h, &mut m, &mut stored, &mut gamma, &mut resets) }, QN_OK, "{}", last_error());
                (m, stored, gamma, resets)
            }
        }
    };
}
lbfgs_memory!(GpuLbfgs);
lbfgs_memory!(GpuProjectedLbfgs);

gpu_solver!(
    /// Orthant-wise limited-memory quasi-Newton (OWL-QN, Andrew and Gao 2007): min f(x) + sum_j l1_j |x_j|, UNBOUNDED ONLY.
    /// `new(tol, x0).with_l1(&l1)` or `.with_l1_scalar(v)`, `.with_memory(m)`; `GpuLbfgs`'s memory and direction kernels applied to the
    /// pseudo-gradient, the direction aligned with it, every trial point projected onto the orthant of x (QN_PATH_LBFGS | QN_PATH_OWLQN);
    /// `GpuBackTracking` only, on the composite value.  The weights the projection switches off are exactly 0.0.  The pairs are differences of
    /// the smooth gradient: `set_l1` between two minimize calls keeps them, x and the memoised evaluation.  Drive it with
    /// `minimize_on_device` / `minimize_objective`: `update_next_iterate` returns `ErrorInputParams`.
    GpuOwlqn, QN_OWLQN, false
);
lbfgs_memory!(GpuOwlqn);

impl GpuOwlqn {
    /// one value per entry, each finite and >= 0; an entry with 0 is smooth
    pub fn with_l1(mut self, l1: &DVector<Floating>) -> Self {
        self.set_l1(l1);
        self
    }
    pub fn with_l1_scalar(mut self, l1: Floating) -> Self {
        self.set_l1_scalar(l1);
        self
    }
    /// between two minimize calls (the regularisation path): the pairs, x and the memoised evaluation are kept
    pub fn set_l1(&mut self, l1: &DVector<Floating>) {
        assert_eq!(l1.len(), self.core.x.len());
        assert_eq!(unsafe { qn_solver_set_l1(self.core.h, l1.as_ptr(), 0.0) }, QN_OK, "{}", last_error());
    }
    pub fn set_l1_scalar(&mut self, l1: Floating) {
        assert_eq!(unsafe { qn_solver_set_l1(self.core.h, std::ptr::null(), l1) }, QN_OK, "{}", last_error());
    }
    pub fn l1(&self) -> DVector<Floating> {
        let mut v = DVector::zeros(self.core.x.len());
        assert_eq!(unsafe { qn_solver_get_l1(self.core.h, v.as_mut_ptr()) }, QN_OK, "{}", last_error());
        v
    }
    /// v of the last loop top
    pub fn pseudo_gradient(&self) -> DVector<Floating> {
        let mut v = DVector::zeros(self.core.x.len());
        assert_eq!(unsafe { qn_solver_get_pseudo_gradient(self.core.h, v.as_mut_ptr()) }, QN_OK, "{}", last_error());
        v
    }
    /// h at x()
    pub fn penalty(&self) -> Floating {
        self.l1().iter().zip(self.core.x.iter()).map(|(w, x)| w * x.abs()).sum()
    }
    pub fn nonzeros(&self) -> usize {
        self.core.x.iter().filter(|v| **v != 0.0).count()
    }
}

gpu_solver!(
    /// Nonlinear conjugate gradient: `new(tol, x0).with_variant(CgVariant::HagerZhang, 0.2, 0)`; d+ = beta d - g+ with one extra vector of state on
    /// the GPU (QN_PATH_CG): the accept pass leaves every inner product beta needs, so the direction costs one stream and no reduction launch of
    /// its own.  Restarts d = -g by Powell's test |g+.g| >= powell_nu g+.g+ (`f64::INFINITY`: off), every `restart_every` iterations (0: never) and
    /// whenever beta d - g+ would not descend.  UNBOUNDED ONLY; `GpuStrongWolfe` (what FR, DY and HS+ assume) or `GpuBackTracking`.  Drive it
    /// with `minimize_on_device` / `minimize_objective`: the direction lives on the device.
    GpuNonlinearCg, QN_NONLINEAR_CG, false
);

gpu_solver!(
    /// Truncated Newton: `new(tol, x0).with_inner(0.5, 0, 8)`; Newton's direction from a few conjugate-gradient steps on H z = g, each costing one
    /// Hessian-vector product of the device log-sum-exp objective (QN_PATH_NEWTON_CG: one stream of A, never a matrix).  UNBOUNDED ONLY;
    /// `DeviceObjective::log_sum_exp` only (n_pad <= 16384); `GpuBackTracking` or `GpuStrongWolfe`, first trial t = 1.  Drive it with
    /// `minimize_objective`: the inner loop lives on the device.
    GpuNewtonCg, QN_NEWTON_CG, false
);

impl GpuNewtonCg {
    /// the forcing term's cap eta_max in (0, 1) (0.5), the inner steps of one direction at the most (0: min(n, 100)), inner steps per batch (8)
    pub fn with_inner(self, eta_max: Floating, max_inner: usize, chunk: usize) -> Self {
        assert_eq!(unsafe { qn_solver_set_newton_cg(self.core.h, eta_max, max_inner, chunk) }, QN_OK, "{}", last_error());
        self
    }
    /// the inner loop's preconditioner: `Preconditioner::None` (the default) or `Preconditioner::Jacobi`, the diagonal of H(x_k) by one more pass
    /// of A per outer iteration.  It pays where the columns of A differ in scale by orders of magnitude; on well-scaled columns, or with m < n
    /// and a small mu, it buys nothing or loses.  Log-sum-exp, logistic and sparse logistic objectives only.
    pub fn preconditioner(self, kind: Preconditioner) -> Self {
        let code = match kind {
            Preconditioner::None => QN_PRECOND_NONE,
            Preconditioner::Jacobi => QN_PRECOND_JACOBI,
        };
        assert_eq!(unsafe { qn_solver_set_newton_cg_preconditioner(self.core.h, code) }, QN_OK, "{}", last_error());
        self
    }
    /// (the setting, directions of the last minimize that started with a diagonal pass, entries of the last 1 / M that were set to 1)
    pub fn precond_state(&self) -> (Preconditioner, usize, usize) {
        let (mut kind, mut passes, mut floored) = (0 as c_int, 0usize, 0usize);
        assert_eq!(unsafe { qn_solver_newton_cg_precond_state(self.core.h, &mut kind, &mut passes, &mut floored) }, QN_OK, "{}", last_error());
        (if kind == QN_PRECOND_JACOBI { Preconditioner::Jacobi } else { Preconditioner::None }, passes, floored)
    }
    /// (inner steps of the last direction, of all directions, Hessian-vector products, non-positive curvature met, rule-8 fallbacks)
    pub fn newton_cg_state(&self) -> (usize, usize, usize, usize, usize) {
        let (mut last, mut total, mut hv, mut neg, mut fb) = (0usize, 0usize, 0usize, 0usize, 0usize);
        assert_eq!(unsafe { qn_solver_newton_cg_state(self.core.h, &mut last, &mut total, &mut hv, &mut neg, &mut fb) }, QN_OK, "{}", last_error());
        (last, total, hv, neg, fb)
    }
}

/// `qn_solver_set_newton_cg_preconditioner`'s kinds
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Preconditioner {
    None,
    Jacobi,
}

/// `qn_solver_set_cg`'s variants
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum CgVariant {
    FletcherReeves,
    PolakRibierePlus,
    HestenesStiefelPlus,
    DaiYuan,
    HagerZhang,
}

impl CgVariant {
    fn code(self) -> c_int {
        match self {
            CgVariant::FletcherReeves => QN_CG_FR,
            CgVariant::PolakRibierePlus => QN_CG_PR_PLUS,
            CgVariant::HestenesStiefelPlus => QN_CG_HS_PLUS,
            CgVariant::DaiYuan => QN_CG_DY,
            CgVariant::HagerZhang => QN_CG_HZ,
        }
    }
    fn from_code(code: c_int) -> Self {
        match code {
            QN_CG_FR => CgVariant::FletcherReeves,
            QN_CG_HS_PLUS => CgVariant::HestenesStiefelPlus,
            QN_CG_DY => CgVariant::DaiYuan,
            QN_CG_HZ => CgVariant::HagerZhang,
            _ => CgVariant::PolakRibierePlus,
        }
    }
}

impl GpuNonlinearCg {
    /// the variant (Polak-Ribiere+ by default), Powell's nu (0.2) and restart_every (0: never); the stored direction is dropped
    pub fn with_variant(self, variant: CgVariant, powell_nu: Floating, restart_every: usize) -> Self {
        assert_eq!(unsafe { qn_solver_set_cg(self.core.h, variant.code(), powell_nu, restart_every) }, QN_OK, "{}", last_error());
        self
    }
    /// (variant, beta of the last accepted iteration, betas that ended as exactly 0, iterations since the last -g direction)
    pub fn cg_state(&self) -> (CgVariant, Floating, usize, usize) {
        let (mut variant, mut beta, mut restarts, mut since) = (0 as c_int, 0.0, 0usize, 0usize);
        assert_eq!(unsafe { qn_solver_cg_state(self.core.h, &mut variant, &mut beta, &mut restarts, &mut since) }, QN_OK, "{}", last_error());
        (CgVariant::from_code(variant), beta, restarts, since)
    }
}

macro_rules! bounded_first_order {
    ($name:ident) => {
        impl $name {
            pub fn with_bounds(mut self, lower_bound: DVector<Floating>, upper_bound: DVector<Floating>) -> Self {
                self.core.set_bounds(lower_bound, upper_bound).expect("qn_solver_set_bounds");
                self
            }
            pub fn grad_tol(&self) -> &Floating {
                &self.core.tol
            }
        }
        impl HasBounds for $name {
            fn lower_bound(&self) -> &DVector<Floating> {
                &self.core.lb
            }
            fn upper_bound(&self) -> &DVector<Floating> {
                &self.core.ub
            }
            fn set_lower_bound(&mut self, lower_bound: DVector<Floating>) {
                let ub = self.core.ub.clone();
                self.core.set_bounds(lower_bound, ub).expect("qn_solver_set_bounds");
            }
            fn set_upper_bound(&mut self, upper_bound: DVector<Floating>) {
                let lb = self.core.lb.clone();
                self.core.set_bounds(lb, upper_bound).expect("qn_solver_set_bounds");
            }
        }
    };
}
bounded_first_order!(GpuProjectedGradientDescent);
bounded_first_order!(GpuSpectralProjectedGradient);
bounded_first_order!(GpuSpectralProximalGradient);
bounded_first_order!(GpuProjectedNewton);
bounded_first_order!(GpuSpectralProjectedNewton);
bounded_first_order!(GpuProjectedLbfgs);
bounded_first_order!(GpuBroydenB); // (the same `with_bounds` / `HasBounds`; `grad_tol()` is its `tol`)

macro_rules! newton_factorisations {
    ($name:ident) => {
        impl $name {
            /// Cholesky factorisations enqueued by the last minimize call (a device quadratic's factor is kept: QN_OPT_PNEWTON_REUSE_FACTOR)
            pub fn newton_factorisations(&self) -> usize {
                let mut v = 0usize;
                unsafe { qn_solver_newton_factorisations(self.core.h, &mut v) };
                v
            }
        }
    };
}
newton_factorisations!(GpuProjectedNewton);
newton_factorisations!(GpuSpectralProjectedNewton);

impl GpuProjectedNewton {
    pub fn s_norm(&self) -> Option<Floating> {
        self.core.option(qn_solver_s_norm)
    }
    pub fn y_norm(&self) -> Option<Floating> {
        self.core.option(qn_solver_y_norm)
    }
    pub fn next_iterate_too_close(&self) -> bool {
        self.core.flag(qn_solver_next_iterate_too_close) // projected_newton.rs:15-20
    }
    pub fn gradient_next_iterate_too_close(&self) -> bool {
        self.core.flag(qn_solver_gradient_next_iterate_too_close) // projected_newton.rs:21-26
    }
}

impl GpuSpectralProjectedNewton {
    /// spn.rs:23-27
    pub fn with_lambdas(self, lambda_min: Floating, lambda_max: Floating) -> Self {
        assert_eq!(unsafe { qn_solver_set_spg_lambdas(self.core.h, lambda_min, lambda_max) }, QN_OK, "{}", last_error());
        self
    }
    pub fn lambda(&self) -> Option<Floating> {
        self.core.option(qn_solver_spg_lambda)
    }
}

gpu_solver!(
    /// Spectral proximal gradient (SpaRSA): min f(x) + sum_j l1_j |x_j| over the box -- `GpuSpectralProjectedGradient` with the projection replaced
    /// by the proximal map of lambda l1 |.| plus the box (QN_PATH_PROX).  `new(tol, x0).with_l1(&l1)` or `.with_l1_scalar(v)`, optionally
    /// `.with_bounds(lb, ub)`; `GpuGllQuadratic` or `GpuBackTracking`, on the composite value.  The weights the prox switches off are exactly 0.0.
    /// The constructor's oracle call (lambda0) is made by the first `minimize_on_device` / `minimize_objective`; drive it with those two.
    GpuSpectralProximalGradient, QN_SPECTRAL_PROXIMAL_GRADIENT, false
);

impl GpuSpectralProximalGradient {
    /// one value per entry, each finite and >= 0
    pub fn with_l1(mut self, l1: &DVector<Floating>) -> Self {
        self.set_l1(l1);
        self
    }
    pub fn with_l1_scalar(mut self, l1: Floating) -> Self {
        self.set_l1_scalar(l1);
        self
    }
    /// between two minimize calls (the regularisation path): GLLQuadratic's ring is cleared; lambda, x and the memoised evaluation are kept
    pub fn set_l1(&mut self, l1: &DVector<Floating>) {
        assert_eq!(l1.len(), self.core.x.len());
        assert_eq!(unsafe { qn_solver_set_l1(self.core.h, l1.as_ptr(), 0.0) }, QN_OK, "{}", last_error());
    }
    pub fn set_l1_scalar(&mut self, l1: Floating) {
        assert_eq!(unsafe { qn_solver_set_l1(self.core.h, std::ptr::null(), l1) }, QN_OK, "{}", last_error());
    }
    pub fn l1(&self) -> DVector<Floating> {
        let mut v = DVector::zeros(self.core.x.len());
        assert_eq!(unsafe { qn_solver_get_l1(self.core.h, v.as_mut_ptr()) }, QN_OK, "{}", last_error());
        v
    }
    pub fn with_lambdas(self, lambda_min: Floating, lambda_max: Floating) -> Self {
        assert_eq!(unsafe { qn_solver_set_spg_lambdas(self.core.h, lambda_min, lambda_max) }, QN_OK, "{}", last_error());
        self
    }
    /// None until the first minimize call has made the constructor's evaluation
    pub fn lambda(&self) -> Option<Floating> {
        self.core.option(qn_solver_spg_lambda)
    }
    /// h at x()
    pub fn penalty(&self) -> Floating {
        self.l1().iter().zip(self.core.x.iter()).map(|(w, x)| w * x.abs()).sum()
    }
    pub fn nonzeros(&self) -> usize {
        self.core.x.iter().filter(|v| **v != 0.0).count()
    }
}

impl GpuSpectralProjectedGradient {
    /// spg.rs:23-27
    pub fn with_lambdas(self, lambda_min: Floating, lambda_max: Floating) -> Self {
        assert_eq!(unsafe { qn_solver_set_spg_lambdas(self.core.h, lambda_min, lambda_max) }, QN_OK, "{}", last_error());
        self
    }
    /// `lambda()`: None until the first minimize call has made the constructor's evaluation
    pub fn lambda(&self) -> Option<Floating> {
        self.core.option(qn_solver_spg_lambda)
    }
}

macro_rules! quasi_newton_getters {
    ($name:ident) => {
        impl $name {
            pub fn s_norm(&self) -> Option<Floating> {
                self.core.option(qn_solver_s_norm)
            }
            pub fn y_norm(&self) -> Option<Floating> {
                self.core.option(qn_solver_y_norm)
            }
            pub fn next_iterate_too_close(&self) -> bool {
                self.core.flag(qn_solver_next_iterate_too_close) // bfgs.rs:15-20
            }
            pub fn gradient_next_iterate_too_close(&self) -> bool {
                self.core.flag(qn_solver_gradient_next_iterate_too_close) // bfgs.rs:21-26
            }
            /// Lazy download (applies the pending rank-2 update first); the reference's getter returns a reference to a
            /// host matrix, this one an owned copy of the device one.
            pub fn approx_inv_hessian(&self) -> DMatrix<Floating> {
                self.core.approx_inv_hessian()
            }
            pub fn identity(&self) -> DMatrix<Floating> {
                DMatrix::identity(self.core.n, self.core.n) // bfgs.rs:9; the GPU solver keeps no copy of it
            }
        }
    };
}
quasi_newton_getters!(GpuBFGS);
quasi_newton_getters!(GpuDFP);
