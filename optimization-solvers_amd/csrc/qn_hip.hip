// qn_hip.hip -- host side of libqn_hip.so: the C ABI of include/qn_hip.h, the request pump that drives the
// device-resident state machine (qn_ctl.h), objectives, and the RCCL exchange for row-sharded runs.
//
// No CPU compute path exists here: every flop of the hot path runs in the kernels of qn_kernels.hip.h.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/qn_hip.h"
#include "qn_kernels.hip.h"

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int status, const std::string& msg) {
    g_err = msg;
    return status;
}
#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess)                                                                              \
            return fail(QN_ABNORMAL_TERMINATION, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)
#define QNCHK(expr)                        \
    do {                                   \
        int _s = (expr);                   \
        if (_s != QN_OK) return _s;        \
    } while (0)

extern "C" const char* qn_last_error_message(void) { return g_err.c_str(); }
extern "C" int qn_abi_version(void) { return QN_ABI_VERSION; }
extern "C" const char* qn_status_string(int status) {
    switch (status) { // Display strings of ls_solver.rs:12-19
    case QN_OK: return "Ok";
    case QN_MAX_ITER_REACHED: return "Max iter reached";
    case QN_OUT_OF_DOMAIN: return "Out of domain";
    case QN_ERROR_INPUT_PARAMS: return "Error in input parameters";
    case QN_ABNORMAL_TERMINATION: return "Abnormal termination";
    default: return "Unknown status";
    }
}

// The host side in parts (round 6): textual includes of this one translation unit, in dependency order.
#include "qn_host_context.hip.h"
#include "qn_host_linesearch.hip.h"
#include "qn_host_objective.hip.h"
#include "qn_host_solver.hip.h"
#include "qn_host_launch.hip.h"
#include "qn_host_rank1.hip.h"
#include "qn_host_pnorm.hip.h"
#include "qn_host_newton.hip.h"
#include "qn_host_minimize.hip.h"
#include "qn_host_blas.hip.h"
// the first-order family (SPG, projected gradient, GLLQuadratic): its kernels are defined behind every existing one
#include "qn_vec.hip.h"
#include "qn_vec_wolfe.hip.h"
#include "qn_host_vec.hip.h"
// the log-sum-exp Hessian (Newton on a device log-sum-exp objective): again behind every existing kernel
#include "qn_lse_hess.hip.h"
// limited-memory BFGS on the first-order family's machine: the two streaming kernels of its compact form, behind every existing kernel
#include "qn_lbfgs.hip.h"
#include "qn_host_lbfgs.hip.h"
// the sparse quadratic objective (CSR; the O(n) solvers' large device objective): behind every existing kernel
#include "qn_sparse.hip.h"
// nonlinear conjugate gradient on the first-order family's machine: its direction and accept kernels, behind every existing kernel
#include "qn_cg.hip.h"
#include "qn_host_cg.hip.h"
// the curvature pass of the device quadratics (q = Q v, v'Qv) and qn_objective_hess_vec: behind every existing kernel
#include "qn_vec_exact.hip.h"
// the log-sum-exp Hessian-vector product (q = H v in one stream of A) and qn_objective_hess_vec_at: behind every existing kernel
#include "qn_lse_hv.hip.h"
// the diagonal of the Hessian of the kinds that share that product (one stream of A with squared entries) and qn_objective_hess_diag_at
#include "qn_hess_diag.hip.h"
// the logistic objective (two launches per evaluation; its Hessian-vector product is the log-sum-exp one's kernels): behind every existing kernel
#include "qn_logistic.hip.h"
#include "qn_host_logistic.hip.h"
// the sparse logistic objective (A and A' in CSR; three launches per evaluation and per Hessian-vector product): behind every existing kernel
#include "qn_sparse_logistic.hip.h"
#include "qn_host_sparse_logistic.hip.h"
// the multinomial objective (one stream of A for K classes; the logistic's and the product's combine kernels fold its shares): behind every existing kernel
#include "qn_multinomial.hip.h"
#include "qn_host_multinomial.hip.h"
// the sparse multinomial objective (A and A' in CSR, two SpMM passes on feature-major copies; five launches per evaluation and per product): behind every existing kernel
#include "qn_sparse_multinomial.hip.h"
#include "qn_host_sparse_multinomial.hip.h"
// truncated Newton (NewtonCG) on the first-order family's machine: conjugate gradients on H z = g with that product, behind every existing kernel
#include "qn_newton_cg.hip.h"
#include "qn_host_newton_cg.hip.h"
// spectral proximal gradient (L1 by soft-thresholding) on the first-order family's machine: its direction, trial and decision kernels, behind every existing kernel
#include "qn_vec_prox.hip.h"
#include "qn_host_prox.hip.h"
// orthant-wise L-BFGS (OWL-QN, L1 with curvature) on the same machine: its element-wise kernels, behind the prox pair whose penalty it shares
#include "qn_vec_owlqn.hip.h"
#include "qn_host_owlqn.hip.h"
