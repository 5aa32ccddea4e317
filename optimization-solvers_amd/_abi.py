"""ctypes declarations for libqn_hip.so (include/qn_hip.h).  Loading fails loudly if the HIP library has not
been built: there is no Python or CPU fallback for any compute on this path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QN_HIP_LIB") or os.path.join(_HERE, "lib", "libqn_hip.so")  # QN_HIP_LIB: diagnostic builds

OK, MAX_ITER_REACHED, OUT_OF_DOMAIN, ERROR_INPUT_PARAMS, ABNORMAL_TERMINATION = range(5)
LS_MORETHUENTE, LS_BACKTRACKING, LS_MORETHUENTE_B, LS_BACKTRACKING_B, LS_GLL_QUADRATIC = 0, 1, 2, 3, 4
LS_NO_SEARCH = 5  # line_search/nosearch.rs
LS_STRONG_WOLFE = 6  # MINPACK-2 dcsrch on the vector machine (no counterpart among the reference's searches)
LS_EXACT_QUADRATIC = 7  # the exact step -g.d / d'Qd on a device quadratic (no counterpart among the reference's searches)
ORACLE_HOST, ORACLE_DEVICE_FN, ORACLE_OBJECTIVE = 0, 1, 2
BFGS, DFP, GRADIENT_DESCENT, NEWTON, SR1, SPG, PROJECTED_GRADIENT, PROJECTED_NEWTON, SPECTRAL_PROJECTED_NEWTON = 0, 1, 2, 3, 4, 5, 6, 7, 8
BROYDEN = 9  # quasi_newton/broyden.rs (BroydenB once bounds are set)
COORDINATE_DESCENT, PNORM_DESCENT = 10, 11  # steepest_descent/coordinate_descent.rs, pnorm_descent.rs
LBFGS = 12  # limited-memory BFGS (ProjectedLBFGS once bounds are set); not the reference's Fortran-backed Lbfgsb
LBFGS_MAX_M = 32
NONLINEAR_CG = 13  # nonlinear conjugate gradient (unbounded only); no counterpart in the reference
NEWTON_CG = 14  # truncated Newton on the log-sum-exp Hessian-vector product (unbounded only); no counterpart in the reference
SPECTRAL_PROXIMAL_GRADIENT = 15  # L1-regularised SPG by soft-thresholding (SpaRSA); no counterpart in the reference
OWLQN = 16  # orthant-wise L-BFGS for L1-regularised objectives (unbounded only); no counterpart in the reference
CG_FR, CG_PR_PLUS, CG_HS_PLUS, CG_DY, CG_HZ = 0, 1, 2, 3, 4  # qn_solver_set_cg's variants
PRECOND_NONE, PRECOND_JACOBI = 0, 1  # qn_solver_set_newton_cg_preconditioner's kinds
UNIQUE_ID_BYTES = 128

dp = C.POINTER(C.c_double)


class LineSearchStruct(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32),
                ("c1", C.c_double), ("c2", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double),
                ("delta_min", C.c_double), ("delta", C.c_double), ("delta_max", C.c_double),
                ("bt_c1", C.c_double), ("bt_beta", C.c_double),
                ("lower_bound_host", C.c_void_p), ("upper_bound_host", C.c_void_p)]


HOST_ORACLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, C.c_size_t, dp, dp)
DEVICE_ORACLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)
CALLBACK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
HOST_HESSIAN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, C.c_size_t, dp)
HOST_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, dp, C.c_size_t)


class OracleStruct(C.Structure):
    _fields_ = [("kind", C.c_int32), ("memoize", C.c_int32),
                ("host_fn", C.c_void_p), ("host_user", C.c_void_p),
                ("device_fn", C.c_void_p), ("device_user", C.c_void_p),
                ("objective", C.c_void_p), ("host_hessian_fn", C.c_void_p)]


class TraceRec(C.Structure):
    _fields_ = [("f", C.c_double), ("gnorm", C.c_double), ("t", C.c_double), ("s_norm", C.c_double), ("y_norm", C.c_double),
                ("n_evals", C.c_int32), ("ls_iters", C.c_int32), ("ls_cases", C.c_int32), ("updated", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_uint64), ("oracle_calls", C.c_uint64), ("oracle_evals", C.c_uint64),
                ("h_passes", C.c_uint64), ("h_bytes", C.c_uint64), ("obj_bytes", C.c_uint64),
                ("launches", C.c_uint64), ("host_syncs", C.c_uint64),
                ("t_hpass_ms", C.c_double), ("t_eval_ms", C.c_double), ("t_ctl_ms", C.c_double), ("t_comm_ms", C.c_double),
                ("n_hpass_timed", C.c_uint64), ("n_eval_timed", C.c_uint64), ("n_ctl_timed", C.c_uint64), ("n_comm_timed", C.c_uint64),
                ("matrix_bytes_per_pass", C.c_uint64),
                ("total_minimize_calls", C.c_uint64), ("total_iterations", C.c_uint64), ("total_oracle_calls", C.c_uint64),
                ("total_oracle_evals", C.c_uint64), ("total_h_passes", C.c_uint64), ("total_h_bytes", C.c_uint64),
                ("total_obj_bytes", C.c_uint64), ("path", C.c_uint32), ("_pad", C.c_uint32),
                ("t_hreduce_ms", C.c_double), ("t_ereduce_ms", C.c_double), ("n_hreduce_timed", C.c_uint64), ("n_ereduce_timed", C.c_uint64),
                ("total_xchg_vector", C.c_uint64), ("total_xchg_scalar", C.c_uint64),
                ("t_newton_ms", C.c_double), ("n_newton_timed", C.c_uint64), ("newton_lu_sync_timeouts", C.c_uint64),
                ("fast_machine_steps", C.c_uint64), ("n_hpass_nostore", C.c_uint64), ("h_bytes_moved", C.c_uint64)]


PATH_FUSED, PATH_SYM, PATH_SYM_GENERIC, PATH_PIPELINED, PATH_SYM2, PATH_TILES1, PATH_VECTOR, PATH_PNEWTON = 1, 2, 4, 8, 16, 32, 64, 128
PATH_RANK1 = 256
PATH_PNORM = 512
PATH_LBFGS = 1024
PATH_CG = 2048
PATH_EXACT = 4096
PATH_NEWTON_CG = 8192
PATH_PROX = 16384
PATH_OWLQN = 32768


# every symbol include/qn_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("qn_status_string", C.c_char_p, [C.c_int]),
    ("qn_last_error_message", C.c_char_p, []),
    ("qn_abi_version", C.c_int, []),
    ("qn_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("qn_context_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("qn_comm_unique_id", C.c_int, [C.c_void_p]),
    ("qn_context_create_sharded", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("qn_context_create_sharded_host_exchange", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("qn_context_destroy", None, [C.c_void_p]),
    ("qn_partition", C.c_int, [C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("qn_comm_selftest", C.c_int, [C.c_void_p]),
    ("qn_context_comm_check", C.c_int, [C.c_void_p]),
    ("qn_context_exchange_probe", C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    ("qn_context_event_bracket_overhead", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    ("qn_context_synchronize", C.c_int, [C.c_void_p]),
    ("qn_context_rank", C.c_int, [C.c_void_p]),
    ("qn_context_world", C.c_int, [C.c_void_p]),
    ("qn_context_stream", C.c_void_p, [C.c_void_p]),
    ("qn_context_set_host_exchange_async", C.c_int, [C.c_void_p, C.c_int]),
    ("qn_context_set_trial_vector_exchange", C.c_int, [C.c_void_p, C.c_int]),
    ("qn_context_set_allreduce", C.c_int, [C.c_void_p, C.c_int]),
    ("qn_morethuente_default", None, [C.POINTER(LineSearchStruct)]),
    ("qn_morethuente_with_deltas", C.c_int, [C.POINTER(LineSearchStruct), C.c_double, C.c_double, C.c_double]),
    ("qn_morethuente_with_t_min", C.c_int, [C.POINTER(LineSearchStruct), C.c_double]),
    ("qn_morethuente_with_t_max", C.c_int, [C.POINTER(LineSearchStruct), C.c_double]),
    ("qn_morethuente_with_c1", C.c_int, [C.POINTER(LineSearchStruct), C.c_double]),
    ("qn_morethuente_with_c2", C.c_int, [C.POINTER(LineSearchStruct), C.c_double]),
    ("qn_backtracking_new", None, [C.POINTER(LineSearchStruct), C.c_double, C.c_double]),
    ("qn_morethuente_b_new", None, [C.POINTER(LineSearchStruct)]),
    ("qn_backtracking_b_new", None, [C.POINTER(LineSearchStruct), C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    ("qn_linesearch_with_lower_bound", None, [C.POINTER(LineSearchStruct), C.c_void_p]),
    ("qn_linesearch_with_upper_bound", None, [C.POINTER(LineSearchStruct), C.c_void_p]),
    ("qn_nosearch_new", None, [C.POINTER(LineSearchStruct)]),
    ("qn_gll_quadratic_new", None, [C.POINTER(LineSearchStruct), C.c_double, C.c_size_t]),
    ("qn_gll_quadratic_with_sigmas", None, [C.POINTER(LineSearchStruct), C.c_double, C.c_double]),
    ("qn_strong_wolfe_new", None, [C.POINTER(LineSearchStruct), C.c_double, C.c_double]),
    ("qn_strong_wolfe_with_xtol", C.c_int, [C.POINTER(LineSearchStruct), C.c_double]),
    ("qn_exact_quadratic_new", None, [C.POINTER(LineSearchStruct), C.c_int]),
    ("qn_quadratic_create", C.c_int, [C.c_void_p, C.c_size_t, dp, dp, C.POINTER(C.c_void_p)]),
    ("qn_quadratic_create_synthetic", C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, dp, dp, C.POINTER(C.c_void_p)]),
    ("qn_logsumexp_create", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, dp, dp, C.c_double, C.POINTER(C.c_void_p)]),
    ("qn_logistic_create", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, dp, dp, dp, C.c_double, C.POINTER(C.c_void_p)]),
    ("qn_sparse_logistic_create", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, dp, dp, dp, C.c_double,
                                            C.POINTER(C.c_void_p)]),
    ("qn_sparse_logistic_set_lanes", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("qn_sparse_logistic_info", C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_size_t)]),
    ("qn_multinomial_create", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, dp, C.c_void_p, dp, C.c_double, C.POINTER(C.c_void_p)]),
    ("qn_multinomial_probabilities", C.c_int, [C.c_void_p, dp, dp]),
    ("qn_multinomial_set_kernel", C.c_int, [C.c_void_p, C.c_int]),
    ("qn_sparse_multinomial_create", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, dp, C.c_void_p,
                                               dp, C.c_double, C.POINTER(C.c_void_p)]),
    ("qn_sparse_multinomial_info", C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    ("qn_sparse_multinomial_set_lanes", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("qn_sparse_multinomial_probabilities", C.c_int, [C.c_void_p, dp, dp]),
    ("qn_sparse_quadratic_create", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, dp, dp, C.POINTER(C.c_void_p)]),
    ("qn_sparse_quadratic_set_lanes_per_row", C.c_int, [C.c_void_p, C.c_int]),
    ("qn_objective_sparse_info", C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    ("qn_objective_destroy", None, [C.c_void_p]),
    ("qn_objective_eval", C.c_int, [C.c_void_p, dp, dp, dp]),
    ("qn_objective_get_rows", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, dp]),
    ("qn_objective_hessian", C.c_int, [C.c_void_p, dp, dp]),
    ("qn_objective_hess_vec", C.c_int, [C.c_void_p, dp, dp, dp]),
    ("qn_objective_hess_vec_at", C.c_int, [C.c_void_p, dp, dp, dp, dp]),
    ("qn_objective_hess_diag_at", C.c_int, [C.c_void_p, dp, dp]),
    ("qn_solver_create", C.c_int, [C.c_void_p, C.c_int, C.c_double, dp, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("qn_solver_destroy", None, [C.c_void_p]),
    ("qn_solver_reset", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_set_bounds", C.c_int, [C.c_void_p, dp, dp]),
    ("qn_solver_set_inverse_p", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_get_inverse_p", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_set_spg_lambdas", C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    ("qn_solver_spg_lambda", C.c_int, [C.c_void_p, dp, C.POINTER(C.c_int)]),
    ("qn_solver_set_l1", C.c_int, [C.c_void_p, dp, C.c_double]),
    ("qn_solver_get_l1", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_get_pseudo_gradient", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_newton_factorisations", C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    ("qn_solver_set_lbfgs_memory", C.c_int, [C.c_void_p, C.c_size_t]),
    ("qn_solver_lbfgs_state", C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), dp, C.POINTER(C.c_size_t)]),
    ("qn_solver_set_cg", C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_size_t]),
    ("qn_solver_cg_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int), dp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("qn_solver_set_newton_cg", C.c_int, [C.c_void_p, C.c_double, C.c_size_t, C.c_size_t]),
    ("qn_solver_newton_cg_state", C.c_int, [C.c_void_p] + [C.POINTER(C.c_size_t)] * 5),
    ("qn_solver_set_newton_cg_preconditioner", C.c_int, [C.c_void_p, C.c_int]),
    ("qn_solver_newton_cg_precond_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("qn_solver_newton_cg_precond_diag", C.c_int, [C.c_void_p, dp, dp]),
    ("qn_solver_exact_state", C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), dp, dp]),
    ("qn_minimize", C.c_int, [C.c_void_p, C.POINTER(LineSearchStruct), C.POINTER(OracleStruct), C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("qn_compute_step_len", C.c_int, [C.c_void_p, C.POINTER(LineSearchStruct), dp, C.c_double, dp, dp, C.c_size_t, C.POINTER(OracleStruct), C.c_size_t,
                             C.POINTER(C.c_double)]),
    ("qn_solver_n", C.c_size_t, [C.c_void_p]),
    ("qn_solver_k", C.c_size_t, [C.c_void_p]),
    ("qn_solver_set_k", C.c_int, [C.c_void_p, C.c_size_t]),
    ("qn_solver_tol", C.c_double, [C.c_void_p]),
    ("qn_solver_get_x", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_set_x", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_get_direction", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_get_gradient", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_s_norm", C.c_int, [C.c_void_p, dp, C.POINTER(C.c_int)]),
    ("qn_solver_y_norm", C.c_int, [C.c_void_p, dp, C.POINTER(C.c_int)]),
    ("qn_solver_next_iterate_too_close", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("qn_solver_gradient_next_iterate_too_close", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("qn_solver_decrement_squared", C.c_int, [C.c_void_p, dp, C.POINTER(C.c_int)]),
    ("qn_solver_get_inv_hessian", C.c_int, [C.c_void_p, dp, C.c_int]),
    ("qn_solver_set_inv_hessian", C.c_int, [C.c_void_p, dp]),
    ("qn_solver_compute_direction", C.c_int, [C.c_void_p, dp, dp]),
    ("qn_solver_secant_update", C.c_int, [C.c_void_p, dp, dp]),
    ("qn_solver_set_trace", C.c_int, [C.c_void_p, C.c_size_t, C.c_int]),
    ("qn_solver_get_trace", C.c_int, [C.c_void_p, C.POINTER(TraceRec), C.c_size_t, C.POINTER(C.c_size_t), dp]),
    ("qn_solver_get_stats", C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    ("qn_solver_set_profiling", C.c_int, [C.c_void_p, C.c_int]),
    ("qn_solver_set_sync_mode", C.c_int, [C.c_void_p, C.c_int]),
    ("qn_solver_set_tiling", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("qn_solver_set_option", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("qn_dev_alloc", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("qn_dev_free", C.c_int, [C.c_void_p, C.c_void_p]),
    ("qn_h2d", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("qn_d2h", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("qn_gemv", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("qn_rank2_update", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                  C.c_double, C.c_double, C.c_double]),
    ("qn_axpy", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    ("qn_dot", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, dp]),
    ("qn_nrm2", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, dp]),
]

_lib = None


def lib():
    """Load libqn_hip.so and bind every declared symbol.  Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback for this path.")
    L = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(L, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L
