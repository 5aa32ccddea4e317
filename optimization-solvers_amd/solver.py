"""Host-side mirror of the reference's trait surface over the C ABI (include/qn_hip.h).

Names, argument meaning and error behaviour follow the Rust crate so the parity tests read like the
reference's own tests:

    BFGS::new(tol, x0)                          -> BFGS(tol, x0)                      (bfgs.rs:27-39)
    MoreThuente::default().with_c1(..)          -> MoreThuente().with_c1(..)          (morethuente.rs:16-62)
    BackTracking::new(c1, beta)                 -> BackTracking(c1, beta)             (backtracking.rs:8-10)
    solver.minimize(&mut ls, oracle, a, b, cb)  -> solver.minimize(ls, oracle, a, b, callback)   (ls_solver.rs:66-111)
    Result<(), SolverError>                     -> returns None / raises SolverError  (ls_solver.rs:10-20)
    FuncEvalMultivariate::new(f, g)             -> FuncEvalMultivariate(f, g) or a plain (f, g) tuple (func_eval.rs:4-41)

Everything numeric happens in libqn_hip.so on the GPU; this file only marshals.
"""
import atexit
import ctypes as C
import weakref

import numpy as np

from . import _abi as A

# Every live handle, so that interpreter exit can release them in dependency order (solvers and objectives before their
# context) instead of whatever order module teardown picks -- a solver destroyed after its context would free device memory
# through a dead stream.
_live = {"solver": weakref.WeakSet(), "objective": weakref.WeakSet(), "context": weakref.WeakSet()}


@atexit.register
def _close_all():
    for kind in ("solver", "objective", "context"):
        for obj in list(_live[kind]):
            try:
                obj.close()
            except Exception:  # noqa: BLE001
                pass


# qn_option (include/qn_hip.h, ABI 5)
OPTIONS = {
    "generic_kernels": 1,
    "deferred_update_step": 2,
    "symmetric_storage": 3,
    "second_generation": 4,
    "folded_accept_reduce": 5,
    "row_slivers": 6,
    "eval_pair_instance": 7,
    "eval_mover_multiplier": 8,
    "tail_reduce": 9,
    "bounded_second_generation": 10,
    "newton_pivoted_lu": 11,
    "lu_per_column_panel": 12,
    "lu_lookahead": 13,
    "lu_one_launch_panel": 14,
    "lu_force_wait_expiry": 15,
    "chunks_per_trip": 16,
    "lu_split_role_a": 17,
    "lu_split_min_rows": 18,
    "btb_project_in_eval": 19,
    "eval_zigzag": 20,
    "touch_h_rows": 21,
    "touch_q_rows": 22,
    "pnewton_reuse_factor": 23,
    "pnorm_nontemporal": 24,
    "pnorm_rows_per_wave": 25,
    "lbfgs_unit_scaling": 26,
    "machine_fast_steps": 27,
    "hpass_store_skip": 28,
}
OPT_GENERIC_KERNELS = 1
OPT_DEFERRED_UPDATE_STEP = 2
OPT_SYMMETRIC_STORAGE = 3
OPT_SECOND_GENERATION = 4
OPT_FOLDED_ACCEPT_REDUCE = 5
OPT_ROW_SLIVERS = 6
OPT_EVAL_PAIR_INSTANCE = 7
OPT_EVAL_MOVER_MULTIPLIER = 8
OPT_TAIL_REDUCE = 9
OPT_BOUNDED_SECOND_GENERATION = 10
OPT_NEWTON_PIVOTED_LU = 11
OPT_LU_PER_COLUMN_PANEL = 12
OPT_LU_LOOKAHEAD = 13
OPT_LU_ONE_LAUNCH_PANEL = 14
OPT_LU_FORCE_WAIT_EXPIRY = 15
OPT_CHUNKS_PER_TRIP = 16
OPT_LU_SPLIT_ROLE_A = 17
OPT_LU_SPLIT_MIN_ROWS = 18
OPT_BTB_PROJECT_IN_EVAL = 19
OPT_EVAL_ZIGZAG = 20
OPT_TOUCH_H_ROWS = 21
OPT_TOUCH_Q_ROWS = 22
OPT_PNEWTON_REUSE_FACTOR = 23
OPT_PNORM_NONTEMPORAL = 24
OPT_PNORM_ROWS_PER_WAVE = 25
OPT_LBFGS_UNIT_SCALING = 26
OPT_MACHINE_FAST_STEPS = 27
OPT_HPASS_STORE_SKIP = 28


class SolverError(Exception):
    """ls_solver.rs:10-20"""
    code = A.ABNORMAL_TERMINATION

    def __init__(self, msg=None):
        super().__init__(msg or A.lib().qn_status_string(self.code).decode())


class MaxIterReached(SolverError):
    code = A.MAX_ITER_REACHED


class OutOfDomain(SolverError):
    code = A.OUT_OF_DOMAIN


class ErrorInputParams(SolverError):
    code = A.ERROR_INPUT_PARAMS


class AbnormalTermination(SolverError):
    code = A.ABNORMAL_TERMINATION


_ERRORS = {A.MAX_ITER_REACHED: MaxIterReached, A.OUT_OF_DOMAIN: OutOfDomain, A.ERROR_INPUT_PARAMS: ErrorInputParams,
           A.ABNORMAL_TERMINATION: AbnormalTermination}


def _check(status):
    if status == A.OK:
        return
    detail = A.lib().qn_last_error_message().decode()
    cls = _ERRORS.get(status, AbnormalTermination)
    if status in (A.ERROR_INPUT_PARAMS, A.ABNORMAL_TERMINATION) and detail:
        raise cls(f"{A.lib().qn_status_string(status).decode()}: {detail}")
    raise cls()


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(A.dp)


class FuncEvalMultivariate:
    """func_eval.rs:4-41 (f, g; the optional Hessian is not used on this path)."""

    def __init__(self, f, g, hessian=None):
        self._f, self._g = float(f), np.asarray(g, dtype=np.float64)
        self._h = hessian

    @classmethod
    def new(cls, f, g):
        return cls(f, g)

    def with_hessian(self, hessian):  # func_eval.rs:27-30
        self._h = np.asarray(hessian, dtype=np.float64)
        return self

    def hessian(self):
        return self._h

    def f(self):
        return self._f

    def g(self):
        return self._g

    def __iter__(self):
        return iter((self._f, self._g))


class Context:
    """One GPU (+ optionally one rank of a row-sharded group)."""

    def __init__(self, device=0, rank=0, world=1, unique_id=None, host_allgather=None):
        L = A.lib()
        self.h = C.c_void_p()
        self._keep = None
        if world == 1:
            _check(L.qn_context_create(device, C.byref(self.h)))
        elif host_allgather is not None:
            def tramp(_u, send, recv, count):
                s = np.ctypeslib.as_array(send, shape=(count,))
                r = np.ctypeslib.as_array(recv, shape=(count * world,))
                try:
                    host_allgather(s, r)
                    return 0
                except Exception:  # noqa: BLE001
                    import traceback
                    traceback.print_exc()
                    return 1
            self._keep = A.HOST_ALLGATHER_FN(tramp)
            _check(L.qn_context_create_sharded_host_exchange(device, rank, world, C.cast(self._keep, C.c_void_p), None, C.byref(self.h)))
        else:
            buf = C.create_string_buffer(bytes(unique_id), A.UNIQUE_ID_BYTES)
            _check(L.qn_context_create_sharded(device, rank, world, buf, C.byref(self.h)))
        self.rank, self.world, self.device = rank, world, device
        _live["context"].add(self)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(A.UNIQUE_ID_BYTES)
        _check(A.lib().qn_comm_unique_id(buf))
        return bytes(buf.raw)

    def synchronize(self):
        _check(A.lib().qn_context_synchronize(self.h))

    def comm_selftest(self):
        _check(A.lib().qn_comm_selftest(self.h))

    def comm_check(self):
        """Collective: one verified rank-tagged all-gather through this context's exchange (RCCL or host-staged)."""
        _check(A.lib().qn_context_comm_check(self.h))

    def exchange_probe(self, count, reps=20):
        """Collective: the latency of one exchange of `count` doubles per rank on this context (qn_context_exchange_probe):
        {"median_us", "min_us", "max_us", "bytes_per_rank"}."""
        out = (C.c_double * 3)()
        _check(A.lib().qn_context_exchange_probe(self.h, int(count), int(reps), out))
        return {"bytes_per_rank": 8 * int(count), "median_us": out[0], "min_us": out[1], "max_us": out[2]}

    def set_allreduce(self, on=True):
        """Sharded symmetric storage: all-reduce the partial n-vectors (RCCL's order) instead of all-gather + rank-order sum."""
        _check(A.lib().qn_context_set_allreduce(self.h, 1 if on else 0))

    def set_trial_vector_exchange(self, on=True):
        """Row-sharded second-generation runs, quadratic objective: every evaluation's collective also carries the rank's partial n-vector of
        the trial point (one grouped all-gather), an accepted evaluation then needs no exchange of its own -- E + 1 collectives per
        iteration instead of E + 2; the same iterates.  Not together with set_allreduce."""
        _check(A.lib().qn_context_set_trial_vector_exchange(self.h, 1 if on else 0))

    def set_host_exchange_async(self, on=True):
        """Host-exchange contexts: run the exchange in stream order (no synchronisation), so sharded runs can be pipelined."""
        _check(A.lib().qn_context_set_host_exchange_async(self.h, 1 if on else 0))

    def event_bracket_overhead_ms(self, reps=200):
        """Mean elapsed time an event / launch / event bracket reports for an empty kernel on the idle stream."""
        out = C.c_double(0.0)
        _check(A.lib().qn_context_event_bracket_overhead(self.h, int(reps), C.byref(out)))
        return out.value

    def close(self):
        if self.h:
            A.lib().qn_context_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def partition(n, world):
    """(rows_per_rank, n_pad) of the row partition used for H and the objective's matrix."""
    rpr, npad = C.c_size_t(), C.c_size_t()
    _check(A.lib().qn_partition(n, world, C.byref(rpr), C.byref(npad)))
    return rpr.value, npad.value


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class _LineSearch:
    """LineSearch (line_search/mod.rs:14-23): `compute_step_len` on its own, as the reference's line-search tests call it."""

    def compute_step_len(self, x_k, eval_x_k, direction_k, oracle, max_iter, ctx=None, memoize=None):
        ctx = ctx or (oracle.ctx if isinstance(oracle, Objective) else default_context())
        x, d = _f64(x_k), _f64(direction_k)
        f0, g0 = (eval_x_k.f(), _f64(eval_x_k.g())) if isinstance(eval_x_k, FuncEvalMultivariate) else (float(eval_x_k[0]), _f64(eval_x_k[1]))
        o = A.OracleStruct()
        keep, err = [], []
        if isinstance(oracle, Objective):
            o.kind = A.ORACLE_OBJECTIVE
            o.objective = oracle.h
            o.memoize = 1 if memoize is None else int(memoize)
        elif isinstance(oracle, DeviceClosure):
            o.kind, o.device_fn, o.device_user = A.ORACLE_DEVICE_FN, oracle.fn, oracle.user
            o.memoize = 0 if memoize is None else int(memoize)
        else:
            def tramp(_u, xp, nn, fp, gp):
                try:
                    res = oracle(np.ctypeslib.as_array(xp, shape=(nn,)).copy())
                    f, g = (res.f(), res.g()) if isinstance(res, FuncEvalMultivariate) else res[:2]
                    fp[0] = float(f)
                    np.ctypeslib.as_array(gp, shape=(nn,))[:] = np.asarray(g, dtype=np.float64)
                    return 0
                except Exception as e:  # noqa: BLE001 -- a panicking closure aborts the run
                    err.append(e)
                    return 1
            cfn = A.HOST_ORACLE_FN(tramp)
            keep.append(cfn)
            o.kind = A.ORACLE_HOST
            o.host_fn = C.cast(cfn, C.c_void_p)
            o.memoize = 0 if memoize is None else int(memoize)
        t = C.c_double(0.0)
        status = A.lib().qn_compute_step_len(ctx.h, C.byref(self.s), x.ctypes.data_as(A.dp), float(f0), g0.ctypes.data_as(A.dp),
                                             d.ctypes.data_as(A.dp), x.size, C.byref(o), int(max_iter), C.byref(t))
        if err:
            raise err[0]
        _check(status)
        return t.value


def _device_dot(a, b, ctx=None):
    """a.b with the library's dot kernel (nalgebra's accumulation order, mod.rs:35,47,55), operands uploaded for the call"""
    ctx = ctx or default_context()
    a, b = _f64(a), _f64(b)
    da, db = DeviceBuffer(ctx, a), DeviceBuffer(ctx, b)
    try:
        return dot(ctx, a.size, da, db)
    finally:
        da.free()
        db.free()


class _WolfeConditions:
    """SufficientDecreaseCondition / CurvatureCondition / WolfeConditions (line_search/mod.rs:25-83) as the reference's line-search
    structs expose them; the dots run on the device.  (The line searches themselves evaluate these tests inside the device state
    machine; these methods exist so that caller code written against the traits keeps working.)"""

    def c1(self):
        return self.s.c1 if self.s.kind in (A.LS_MORETHUENTE, A.LS_MORETHUENTE_B) else self.s.bt_c1

    def c2(self):
        return self.s.c2

    def sufficient_decrease(self, f_k, f_kp1, grad_k, t, direction_k):  # mod.rs:27-36
        return f_kp1 - f_k <= self.c1() * t * _device_dot(grad_k, direction_k)

    def curvature_condition(self, grad_k, grad_kp1, direction_k):  # mod.rs:41-48
        return _device_dot(grad_kp1, direction_k) >= self.c2() * _device_dot(grad_k, direction_k)

    def strong_curvature_condition(self, grad_k, grad_kp1, direction_k):  # mod.rs:49-56
        return abs(_device_dot(grad_kp1, direction_k)) <= self.c2() * abs(_device_dot(grad_k, direction_k))

    def wolfe_conditions_with_directional_derivative(self, f_k, f_kp1, grad_k, grad_kp1, t, direction_k):  # mod.rs:60-71
        return self.sufficient_decrease(f_k, f_kp1, grad_k, t, direction_k) and self.curvature_condition(grad_k, grad_kp1, direction_k)

    def strong_wolfe_conditions_with_directional_derivative(self, f_k, f_kp1, grad_k, grad_kp1, t, direction_k):  # mod.rs:72-83
        return (self.sufficient_decrease(f_k, f_kp1, grad_k, t, direction_k)
                and self.strong_curvature_condition(grad_k, grad_kp1, direction_k))


class MoreThuente(_LineSearch, _WolfeConditions):
    """morethuente.rs:6-62"""

    def __init__(self):
        self.s = A.LineSearchStruct()
        A.lib().qn_morethuente_default(C.byref(self.s))

    @classmethod
    def default(cls):
        return cls()

    def with_deltas(self, delta_min, delta, delta_max):
        _check(A.lib().qn_morethuente_with_deltas(C.byref(self.s), delta_min, delta, delta_max))
        return self

    def with_t_min(self, t_min):
        _check(A.lib().qn_morethuente_with_t_min(C.byref(self.s), t_min))
        return self

    def with_t_max(self, t_max):
        _check(A.lib().qn_morethuente_with_t_max(C.byref(self.s), t_max))
        return self

    def with_c1(self, c1):
        _check(A.lib().qn_morethuente_with_c1(C.byref(self.s), c1))
        return self

    def with_c2(self, c2):
        _check(A.lib().qn_morethuente_with_c2(C.byref(self.s), c2))
        return self


class BackTracking(_LineSearch, _WolfeConditions):
    """backtracking.rs:3-11 (implements SufficientDecreaseCondition only, backtracking.rs:13-18: `c2` is not meaningful here)"""

    def __init__(self, c1, beta):
        self.s = A.LineSearchStruct()
        A.lib().qn_backtracking_new(C.byref(self.s), c1, beta)

    @classmethod
    def new(cls, c1, beta):
        return cls(c1, beta)


class NoSearch(_LineSearch):
    """nosearch.rs: `compute_step_len` returns 1.0 and never calls the oracle -- how the reference writes a pure Newton step.  Pairs with
    GradientDescent, Newton, CoordinateDescent and PnormDescent (the solvers on the trait's default update hook)."""

    def __init__(self):
        self.s = A.LineSearchStruct()
        A.lib().qn_nosearch_new(C.byref(self.s))

    @classmethod
    def new(cls):
        return cls()


class MoreThuenteB(MoreThuente):
    """morethuente_b.rs: More-Thuente whose t_max is clipped to the box (and stays clipped)."""

    def __init__(self, n):
        self.s = A.LineSearchStruct()
        A.lib().qn_morethuente_b_new(C.byref(self.s))
        self.n = n
        self._lb = self._ub = None

    @classmethod
    def new(cls, n):
        return cls(n)

    def with_lower_bound(self, lb):
        self._lb = _f64(lb)
        A.lib().qn_linesearch_with_lower_bound(C.byref(self.s), self._lb.ctypes.data)
        return self

    def with_upper_bound(self, ub):
        self._ub = _f64(ub)
        A.lib().qn_linesearch_with_upper_bound(C.byref(self.s), self._ub.ctypes.data)
        return self

    def t_max(self):
        return self.s.t_max


class BackTrackingB(_LineSearch):
    """backtracking_b.rs: projected trial points, modified Armijo rule."""

    def __init__(self, c1, beta, lower_bound, upper_bound):
        self.s = A.LineSearchStruct()
        self._lb, self._ub = _f64(lower_bound), _f64(upper_bound)
        A.lib().qn_backtracking_b_new(C.byref(self.s), c1, beta, self._lb.ctypes.data, self._ub.ctypes.data)

    @classmethod
    def new(cls, c1, beta, lower_bound, upper_bound):
        return cls(c1, beta, lower_bound, upper_bound)


class GLLQuadratic(_LineSearch):
    """gll_quadratic.rs: the non-monotone line search of Grippo, Lampariello and Lucidi with a safeguarded quadratic interpolation, for
    SpectralProjectedGradient / ProjectedGradientDescent.  m is the look-back (1: monotone Armijo), at most 64.  The history `f_previous`
    lives in the SOLVER on the device (this object is plain data): it survives successive minimize calls on one solver, `reset` empties it."""

    def __init__(self, c1, m):
        self.s = A.LineSearchStruct()
        A.lib().qn_gll_quadratic_new(C.byref(self.s), float(c1), int(m))

    @classmethod
    def new(cls, c1, m):
        return cls(c1, m)

    def with_sigmas(self, sigma1, sigma2):
        A.lib().qn_gll_quadratic_with_sigmas(C.byref(self.s), float(sigma1), float(sigma2))
        return self

    def c1(self):
        return self.s.c1

    def m(self):
        return self.s._pad


class ExactQuadratic(_LineSearch):
    """The exact step t = -g.d / d'Qd on a device quadratic (Quadratic, SparseQuadratic) for SpectralProjectedGradient, ProjectedGradientDescent,
    LBFGS / ProjectedLBFGS and NonlinearCG -- with NonlinearCG, linear conjugate gradients.  One product Q d per iteration; no value of f is compared.
    refresh_every = 1: the objective evaluates every accepted point (two matrix passes per iteration); k > 1: every k-th; 0: never -- (f, g) of the
    accepted point come from g + t Q d and f + t (g.d + t/2 d'Qd) -- except that convergence is only declared on a gradient the objective evaluated.
    With a box on the solver the step is capped at 1.  Closures, LogSumExp, other solvers, compute_step_len: ErrorInputParams."""

    def __init__(self, refresh_every=1):
        self.s = A.LineSearchStruct()
        A.lib().qn_exact_quadratic_new(C.byref(self.s), int(refresh_every))

    @classmethod
    def new(cls, refresh_every=1):
        return cls(refresh_every)

    def refresh_every(self):
        return self.s._pad


class StrongWolfe(_LineSearch, _WolfeConditions):
    """The strong-Wolfe line search of the O(n) solvers (SpectralProjectedGradient, ProjectedGradientDescent, ProjectedNewton, SpectralProjectedNewton,
    LBFGS / ProjectedLBFGS): MINPACK-2 `dcsrch` / `dcstep` (More' and Thuente 1994), one oracle call per trial.  c1 = ftol, c2 = gtol; xtol 0.1,
    t_min 0, t_max 1e10.  0 < c1 < c2 < 1 is checked by `minimize` (ErrorInputParams).  With a box of its own (`with_lower_bound` / `with_upper_bound`)
    every search is clipped to it: stpmax = min(t_max, the largest step that stays inside); `t_max` itself is never modified.  On a free L-BFGS run
    the curvature condition keeps s.y > 0, so every pair is committed.  g.d >= 0 at the start of a search: AbnormalTermination, x unchanged."""

    def __init__(self, c1=1e-4, c2=0.9):
        self.s = A.LineSearchStruct()
        A.lib().qn_strong_wolfe_new(C.byref(self.s), float(c1), float(c2))
        self._lb = self._ub = None

    @classmethod
    def new(cls, c1=1e-4, c2=0.9):
        return cls(c1, c2)

    def with_xtol(self, xtol):
        _check(A.lib().qn_strong_wolfe_with_xtol(C.byref(self.s), float(xtol)))
        return self

    def with_t_min(self, t_min):
        _check(A.lib().qn_morethuente_with_t_min(C.byref(self.s), float(t_min)))
        return self

    def with_t_max(self, t_max):
        _check(A.lib().qn_morethuente_with_t_max(C.byref(self.s), float(t_max)))
        return self

    def with_lower_bound(self, lb):
        self._lb = _f64(lb)
        A.lib().qn_linesearch_with_lower_bound(C.byref(self.s), self._lb.ctypes.data)
        return self

    def with_upper_bound(self, ub):
        self._ub = _f64(ub)
        A.lib().qn_linesearch_with_upper_bound(C.byref(self.s), self._ub.ctypes.data)
        return self

    def c1(self):
        return self.s.c1

    def xtol(self):
        return self.s.delta

    def t_min(self):
        return self.s.t_min

    def t_max(self):
        return self.s.t_max


class Objective:
    """A device-resident objective owned by the library."""

    def __init__(self, ctx, handle, n):
        self.ctx, self.h, self.n = ctx, handle, n
        _live["objective"].add(self)

    def __call__(self, x):
        x = _f64(x)
        g = np.empty(self.n)
        f = C.c_double()
        _check(A.lib().qn_objective_eval(self.h, _dp(x), C.byref(f), _dp(g)))
        return FuncEvalMultivariate(f.value, g)

    def hessian(self, x, download=True):
        """The Hessian at x, n x n (`FuncEval::hessian()`): Q for a quadratic; for LogSumExp the matrix the device kernel forms for Newton.
        download=False: the launches run and are waited for, nothing comes back (timing)."""
        x = _f64(x)
        if x.size != self.n:
            raise ErrorInputParams(f"x has {x.size} entries, the objective has {self.n}")
        if not download:
            _check(A.lib().qn_objective_hessian(self.h, _dp(x), None))
            return None
        out = np.empty((self.n, self.n), order="F")
        _check(A.lib().qn_objective_hessian(self.h, _dp(x), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def hess_vec(self, v, download=True):
        """(Q v, v'Qv) of a Quadratic or a SparseQuadratic: one pass over the matrix, no evaluation of f -- the cost of the exact step
        -g.d / d'Qd along d.  download=False: (None, v'Qv).  LogSumExp, Logistic: ErrorInputParams (their Hessian depends on x: hess_vec_at)."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        v = _f64(v)
        if v.size != self.n:
            raise ErrorInputParams(f"v has {v.size} entries, the objective has {self.n}")
        q = np.empty(self.n) if download else None
        c = C.c_double()
        _check(A.lib().qn_objective_hess_vec(self.h, _dp(v), _dp(q) if download else None, C.byref(c)))
        return q, c.value

    def hess_vec_at(self, x, v, download=True):
        """(H(x) v, v'H(x)v) without the matrix.  LogSumExp: the softmax weights at x (two passes of A), then ONE stream of A for
        A'(p o (A v)) - gbar (p . (A v)) + mu v -- the bytes of one evaluation; n_pad <= 16384, one rank (otherwise ErrorInputParams, "not built").
        Logistic: the weights d_i = w_i s_i (1 - s_i) at x (ONE pass of A), then one stream of A for A'(d o (A v)) + mu v.
        SparseLogistic: the same product on the two CSR copies -- a weights pass at x, a row pass over A, a column pass over A', a fold; any n.
        Quadratic / SparseQuadratic: x is not read and the call is `hess_vec(v)`, bit for bit.  download=False: (None, v'Hv)."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        x, v = _f64(x), _f64(v)
        if x.size != self.n:
            raise ErrorInputParams(f"x has {x.size} entries, the objective has {self.n}")
        if v.size != self.n:
            raise ErrorInputParams(f"v has {v.size} entries, the objective has {self.n}")
        q = np.empty(self.n) if download else None
        c = C.c_double()
        _check(A.lib().qn_objective_hess_vec_at(self.h, _dp(x), _dp(v), _dp(q) if download else None, C.byref(c)))
        return q, c.value

    def hess_diag_at(self, x):
        """diag H(x), n entries, without the matrix: the weights at x, then one pass over A with squared entries.  Logistic: sum_i d_i a_ij^2 + mu;
        LogSumExp: sum_i p_i a_ij^2 - gbar_j^2 + mu (n_pad <= 16384, one rank; otherwise ErrorInputParams, "not built"); SparseLogistic: the same sum
        over the device's copy of A' in one launch, any n (an empty column gives mu).  Multinomial, SparseMultinomial, Quadratic, SparseQuadratic:
        ErrorInputParams (not built).  Fixed summation orders: the same bits from call to call and from object to object."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        x = _f64(x)
        if x.size != self.n:
            raise ErrorInputParams(f"x has {x.size} entries, the objective has {self.n}")
        d = np.empty(self.n)
        _check(A.lib().qn_objective_hess_diag_at(self.h, _dp(x), _dp(d)))
        return d

    def rows(self, row0, nrows):
        out = np.empty((nrows, self.n))
        _check(A.lib().qn_objective_get_rows(self.h, row0, nrows, _dp(out)))
        return out

    def close(self):
        if self.h:
            A.lib().qn_objective_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class DeviceClosure:
    """`qn_oracle.kind = QN_ORACLE_DEVICE_FN` (include/qn_hip.h): the caller's own objective, already on the GPU.  `fn` is the
    address of a `qn_device_oracle_fn` -- int fn(void* user, void* stream, const double* x_dev, size_t n, double* f_dev,
    double* g_dev) -- that ENQUEUES its work on `stream`; the solver never copies x, f or g to the host on this path.  It stands
    where the reference takes `impl FnMut(&DVector<f64>) -> FuncEvalMultivariate` (ls_solver.rs:69); like a host closure it is
    called in the reference's order unless `solver.memoize = 1` declares it a pure function of x."""

    def __init__(self, fn, user=None, keep=None):
        self.fn = C.cast(fn, C.c_void_p)
        self.user = C.c_void_p(user) if not isinstance(user, C.c_void_p) else user
        self.keep = keep  # whatever owns `fn` / `user` (a ctypes.CDLL, a create/destroy pair): kept alive with the closure

    @classmethod
    def from_library(cls, path, symbol, user=None):
        dll = C.CDLL(path)
        return cls(getattr(dll, symbol), user, keep=dll)


class Quadratic(Objective):
    """f = 1/2 x'Qx - b'x on the device."""

    def __init__(self, q, b, ctx=None):
        ctx = ctx or default_context()
        q, b = _f64(q), _f64(b)
        h = C.c_void_p()
        _check(A.lib().qn_quadratic_create(ctx.h, b.size, _dp(q), _dp(b), C.byref(h)))
        super().__init__(ctx, h, b.size)

    @classmethod
    def synthetic(cls, n, seed, diag, b, ctx=None):
        ctx = ctx or default_context()
        diag, b = _f64(diag), _f64(b)
        h = C.c_void_p()
        _check(A.lib().qn_quadratic_create_synthetic(ctx.h, n, seed, _dp(diag), _dp(b), C.byref(h)))
        self = cls.__new__(cls)
        Objective.__init__(self, ctx, h, n)
        return self


class SparseQuadratic(Objective):
    """f = 1/2 x'Qx - b'x on the device with a sparse Q in CSR (both triangles of a symmetric matrix; the columns of a row strictly increasing): the
    objective that exists at the sizes the O(n) solvers are for -- SpectralProjectedGradient, ProjectedGradientDescent, LBFGS / ProjectedLBFGS.
    int32 or int64 index arrays are passed through as they are (one width for both: a mixed pair goes as int64), other integer types as int64."""

    def __init__(self, indptr, indices, data, b, ctx=None):
        ctx = ctx or default_context()
        indptr, indices = np.asarray(indptr), np.asarray(indices)
        if indptr.dtype.kind not in "iu" or (indices.size and indices.dtype.kind not in "iu"):
            raise ErrorInputParams("indptr and indices must be integer arrays")
        it = indptr.dtype if indptr.dtype == indices.dtype and indptr.dtype in (np.dtype(np.int32), np.dtype(np.int64)) else np.dtype(np.int64)
        indptr, indices = np.ascontiguousarray(indptr, dtype=it), np.ascontiguousarray(indices, dtype=it)
        data, b = _f64(data), _f64(b)
        if indptr.ndim != 1 or indices.ndim != 1 or data.ndim != 1 or b.ndim != 1 or indptr.size != b.size + 1 or indices.size != data.size:
            raise ErrorInputParams("CSR arrays do not match: indptr has n + 1 entries, indices and data nnz each, b has n")
        # (an empty array's pointer may be null, which the library takes for a missing argument)
        ci = indices if indices.size else np.zeros(1, dtype=it)
        va = data if data.size else np.zeros(1)
        h = C.c_void_p()
        _check(A.lib().qn_sparse_quadratic_create(ctx.h, b.size, data.size, indptr.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                                  it.itemsize, _dp(va), _dp(b), C.byref(h)))
        super().__init__(ctx, h, b.size)

    @classmethod
    def from_scipy(cls, a, b, ctx=None):
        """Any scipy sparse matrix: through .tocsr() with sorted indices and duplicates summed."""
        import scipy.sparse  # noqa: F401 -- only this method needs scipy
        a = a.tocsr().copy()
        a.sum_duplicates()
        a.sort_indices()
        if a.shape[0] != a.shape[1]:
            raise ErrorInputParams(f"Q must be square, got {a.shape}")
        return cls(a.indptr, a.indices, a.data, b, ctx=ctx)

    def __call__(self, x):
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        if np.size(x) != self.n:
            raise ErrorInputParams(f"x has {np.size(x)} entries, the objective has {self.n}")
        return super().__call__(x)

    def _info(self):
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        nnz, lanes, nlong, sym = C.c_size_t(), C.c_int(), C.c_size_t(), C.c_int()
        _check(A.lib().qn_objective_sparse_info(self.h, C.byref(nnz), C.byref(lanes), C.byref(nlong), C.byref(sym)))
        return nnz.value, lanes.value, nlong.value, sym.value

    @property
    def nnz(self):
        return self._info()[0]

    @property
    def lanes_per_row(self):
        return self._info()[1]

    @property
    def n_long_rows(self):
        return self._info()[2]

    @property
    def symmetric(self):
        return self._info()[3]

    def set_lanes_per_row(self, lanes):
        """Lanes that share one row: 1, 2, 4, 8, 16, 32 or 64; 0: chosen from the mean row length.  Another value may change the bits of f and g."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        _check(A.lib().qn_sparse_quadratic_set_lanes_per_row(self.h, int(lanes)))


class LogSumExp(Objective):
    """f = log sum_i exp(a_i'x + c_i) + mu/2 ||x||^2 on the device (A is m x n row-major, rows sharded over ranks).

    A row with c_i = -inf is masked: it contributes nothing to f and g, wherever it falls in the partition of the rows over ranks and workgroups (the
    value is that of the problem with the row deleted).  With every row masked f = -inf + mu/2 ||x||^2, which the line searches treat as non-finite.
    +inf and NaN entries of c and non-finite entries of A are not supported: the result is unspecified."""

    def __init__(self, a, c, mu, ctx=None):
        ctx = ctx or default_context()
        a, c = _f64(a), _f64(c)
        m, n = a.shape
        h = C.c_void_p()
        _check(A.lib().qn_logsumexp_create(ctx.h, m, n, _dp(a), _dp(c), float(mu), C.byref(h)))
        super().__init__(ctx, h, n)
        self.m = m


class Logistic(Objective):
    """Regularised logistic regression on the device: f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2 with a dense A (m x n row-major),
    g = -A'(y o w o s) + mu x, s_i = 1 / (1 + exp(y_i a_i'x)), H = A' diag(d) A + mu I with d_i = w_i s_i (1 - s_i).

    LABELS: every y_i is exactly -1 or +1.  Callers with 0 / 1 labels pass 2 y - 1; any other value is ErrorInputParams -- a 0 never masks a row silently.
    MASKING: `weights` are sample weights >= 0 (default: ones; negative or non-finite: ErrorInputParams).  A row with weight 0 is masked: it adds nothing
    to f, g or H wherever it falls in the cut of the rows over workgroups -- the value is that of the problem with the row deleted.

    One evaluation is two launches and one stream of A, stable for every finite margin.  It runs under SpectralProjectedGradient,
    ProjectedGradientDescent, LBFGS / ProjectedLBFGS, NonlinearCG and NewtonCG; `hess_vec_at(x, v)` gives (H(x) v, v'H(x)v) in one weights pass and one
    product pass of A.  n_pad <= 16384, one rank (otherwise ErrorInputParams, "not built"); `hessian` and `hess_vec`: ErrorInputParams."""

    def __init__(self, a, y, mu, weights=None, ctx=None):
        ctx = ctx or default_context()
        a, y = _f64(a), _f64(y)
        if a.ndim != 2 or y.ndim != 1 or a.shape[0] != y.size:
            raise ErrorInputParams("a must be m x n and y must have m entries")
        m, n = a.shape
        w = None if weights is None else _f64(weights)
        if w is not None and (w.ndim != 1 or w.size != m):
            raise ErrorInputParams(f"weights has {w.size} entries, a has {m} rows")
        h = C.c_void_p()
        _check(A.lib().qn_logistic_create(ctx.h, m, n, _dp(a), _dp(y), _dp(w) if w is not None else None, float(mu), C.byref(h)))
        super().__init__(ctx, h, n)
        self.m = m


class Multinomial(Objective):
    """Regularised softmax (multinomial logistic) regression on the device, with a dense A (m x n row-major), labels y_i in {0, .., K-1} and K =
    `n_classes` >= 2.  The parameter vector is CLASS-MAJOR: x[k n + j] = W[k, j], N = K n entries (sklearn's `coef_` raveled); g and H v use the same
    layout and `self.n` is N.
        f = sum_i w_i (logsumexp_k a_i.W_k - a_i.W_{y_i}) + mu/2 ||x||^2,   g_k = sum_i w_i (p_ik - [y_i = k]) a_i + mu W_k
        (H v)_k = sum_i w_i p_ik (u_ik - sum_l p_il u_il) a_i + mu V_k,   u_ik = a_i.V_k

    LABELS: integers in [0, K); anything else (K, -1, 1.5) is ErrorInputParams with the index.  A class no row carries is legal.
    MASKING: `weights` are sample weights >= 0 (default: ones; negative or non-finite: ErrorInputParams).  A row with weight 0 adds nothing to f, g or H.

    One evaluation is two launches and ONE stream of A for all K classes, stable for every finite margin.  It runs under SpectralProjectedGradient,
    ProjectedGradientDescent, LBFGS / ProjectedLBFGS, NonlinearCG and NewtonCG; `hess_vec_at(x, v)` gives (H(x) v, v'H(x)v) in one weights pass and
    one product pass; `probabilities(x)` the m x K matrix P; `set_kernel` selects the kernel that streams A.  Padded K n <= 16384, K <= 256, one rank (otherwise ErrorInputParams, "not built");
    `hessian`, `hess_vec` and `rows`: ErrorInputParams."""

    def __init__(self, a, y, n_classes, mu, weights=None, ctx=None):
        ctx = ctx or default_context()
        a = _f64(a)
        yf = np.asarray(y, dtype=np.float64)
        if a.ndim != 2 or yf.ndim != 1 or a.shape[0] != yf.size:
            raise ErrorInputParams("a must be m x n and y must have m entries")
        m, n = a.shape
        k = int(n_classes)
        bad = np.flatnonzero(~((yf >= 0) & (yf < max(k, 0)) & (yf == np.floor(yf))))
        if bad.size:
            raise ErrorInputParams(f"multinomial: labels[{int(bad[0])}] = {yf[bad[0]]} is not an integer in [0, n_classes)")
        lab = np.ascontiguousarray(yf, dtype=np.int32)
        w = None if weights is None else _f64(weights)
        if w is not None and (w.ndim != 1 or w.size != m):
            raise ErrorInputParams(f"weights has {w.size} entries, a has {m} rows")
        h = C.c_void_p()
        _check(A.lib().qn_multinomial_create(ctx.h, m, n, max(k, 0), _dp(a), lab.ctypes.data_as(C.c_void_p), _dp(w) if w is not None else None, float(mu),
                                             C.byref(h)))
        super().__init__(ctx, h, n * k)
        self.m, self.n_features, self.n_classes = m, n, k

    def probabilities(self, x):
        """P at x, m x K: P[i, k] = p_ik (a masked row's are zeros).  One weights pass of A."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        x = _f64(x)
        if x.size != self.n:
            raise ErrorInputParams(f"x has {x.size} entries, the objective has {self.n}")
        p = np.empty((self.m, self.n_classes))
        _check(A.lib().qn_multinomial_probabilities(self.h, _dp(x), _dp(p)))
        return p

    def set_kernel(self, kernel):
        """Which kernel streams A: 1 the register-blocked kernel on the vector unit, 2 the MFMA kernel (K <= 64 where it is built, otherwise
        ErrorInputParams), 0 the automatic choice.  The two sum in different orders: each is repeatable bit for bit, not equal to the other."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        _check(A.lib().qn_multinomial_set_kernel(self.h, int(kernel)))


class SparseLogistic(Objective):
    """Regularised logistic regression on the device with a SPARSE A in CSR (m x n; the columns of a row strictly increasing) and no limit on n:
    f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2, g = -A'(y o w o s) + mu x, H(x) v = A'(d o (A v)) + mu v.  Labels (exactly -1 / +1), `weights`
    (>= 0, finite; a 0 masks its row) and mu (finite) follow `Logistic`'s rules.

    The device keeps A AND A' (the host transposes at creation): 24 bytes per nonzero.  The transpose product walks the rows of A' with the kernel
    that walks the rows of A -- no float atomics, every sum in one fixed order, the same bits from run to run and from object to object.  A dense
    column (an intercept column of ones) is a long row of A' and gets a whole workgroup.  One evaluation is three launches; it runs under
    SpectralProjectedGradient, ProjectedGradientDescent, LBFGS / ProjectedLBFGS, NonlinearCG and NewtonCG; `hess_vec_at(x, v)` gives
    (H(x) v, v'H(x)v).  One rank; `hessian`, `hess_vec` and `rows`: ErrorInputParams.
    int32 or int64 index arrays are passed through as they are (one width for both: a mixed pair goes as int64), other integer types as int64."""

    def __init__(self, indptr, indices, data, y, mu, n, weights=None, ctx=None):
        ctx = ctx or default_context()
        indptr, indices = np.asarray(indptr), np.asarray(indices)
        if indptr.dtype.kind not in "iu" or (indices.size and indices.dtype.kind not in "iu"):
            raise ErrorInputParams("indptr and indices must be integer arrays")
        it = indptr.dtype if indptr.dtype == indices.dtype and indptr.dtype in (np.dtype(np.int32), np.dtype(np.int64)) else np.dtype(np.int64)
        indptr, indices = np.ascontiguousarray(indptr, dtype=it), np.ascontiguousarray(indices, dtype=it)
        data, y = _f64(data), _f64(y)
        if indptr.ndim != 1 or indices.ndim != 1 or data.ndim != 1 or y.ndim != 1 or indptr.size != y.size + 1 or indices.size != data.size:
            raise ErrorInputParams("CSR arrays do not match: indptr has m + 1 entries, indices and data nnz each, y has m")
        m = y.size
        w = None if weights is None else _f64(weights)
        if w is not None and (w.ndim != 1 or w.size != m):
            raise ErrorInputParams(f"weights has {w.size} entries, a has {m} rows")
        # (an empty array's pointer may be null, which the library takes for a missing argument)
        ci = indices if indices.size else np.zeros(1, dtype=it)
        va = data if data.size else np.zeros(1)
        h = C.c_void_p()
        _check(A.lib().qn_sparse_logistic_create(ctx.h, m, int(n), data.size, indptr.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                                 it.itemsize, _dp(va), _dp(y), _dp(w) if w is not None else None, float(mu), C.byref(h)))
        super().__init__(ctx, h, int(n))
        self.m = m

    @classmethod
    def from_scipy(cls, a, y, mu, weights=None, ctx=None):
        """Any scipy sparse matrix (m x n): through .tocsr() with sorted indices and duplicates summed."""
        import scipy.sparse  # noqa: F401 -- only this method needs scipy
        a = a.tocsr().copy()
        a.sum_duplicates()
        a.sort_indices()
        return cls(a.indptr, a.indices, a.data, y, mu, a.shape[1], weights=weights, ctx=ctx)

    def __call__(self, x):
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        if np.size(x) != self.n:
            raise ErrorInputParams(f"x has {np.size(x)} entries, the objective has {self.n}")
        return super().__call__(x)

    def _info(self):
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        nnz, lr, lc, nlr, nlc = C.c_size_t(), C.c_int(), C.c_int(), C.c_size_t(), C.c_size_t()
        _check(A.lib().qn_sparse_logistic_info(self.h, C.byref(nnz), C.byref(lr), C.byref(lc), C.byref(nlr), C.byref(nlc)))
        return nnz.value, (lr.value, lc.value), nlr.value, nlc.value

    @property
    def nnz(self):
        return self._info()[0]

    @property
    def lanes(self):
        """(lanes per row of the row pass over A, of the column pass over A')"""
        return self._info()[1]

    @property
    def n_long_rows(self):
        return self._info()[2]

    @property
    def n_long_cols(self):
        return self._info()[3]

    def set_lanes(self, rows, cols):
        """Lanes that share one row of A (`rows`) and one row of A' (`cols`): 1, 2, 4, 8, 16, 32 or 64; 0: chosen from that copy's mean row length.
        Another value may change the bits of f, g and H v."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        _check(A.lib().qn_sparse_logistic_set_lanes(self.h, int(rows), int(cols)))


class SparseMultinomial(Objective):
    """Regularised softmax regression on the device with a SPARSE A in CSR (m x n; the columns of a row strictly increasing): `Multinomial`'s function,
    labels (integers in [0, K), the failing index named), `weights` (>= 0, finite; a 0 masks its row), mu (finite) and CLASS-MAJOR parameter vector
    x[k n + j] = W[k, j] -- `self.n` is N = K n -- with no limit on K n and none on K.

    The device keeps A AND A' (24 bytes per nonzero) and works on feature-major copies with the padded leading dimension `kp`: both halves of an
    evaluation are a sparse matrix times a skinny dense one.  No float atomics, every sum in one fixed order: the same bits from run to run, from
    object to object and for int32 and int64 indices.  One evaluation is five launches; it runs under SpectralProjectedGradient,
    ProjectedGradientDescent, LBFGS / ProjectedLBFGS, NonlinearCG and NewtonCG; `hess_vec_at(x, v)` gives (H(x) v, v'H(x)v); `probabilities(x)` the
    m x K matrix P.  One rank; `hessian`, `hess_vec` and `rows`: ErrorInputParams."""

    def __init__(self, indptr, indices, data, y, n_classes, mu, n, weights=None, ctx=None):
        ctx = ctx or default_context()
        indptr, indices = np.asarray(indptr), np.asarray(indices)
        if indptr.dtype.kind not in "iu" or (indices.size and indices.dtype.kind not in "iu"):
            raise ErrorInputParams("indptr and indices must be integer arrays")
        it = indptr.dtype if indptr.dtype == indices.dtype and indptr.dtype in (np.dtype(np.int32), np.dtype(np.int64)) else np.dtype(np.int64)
        indptr, indices = np.ascontiguousarray(indptr, dtype=it), np.ascontiguousarray(indices, dtype=it)
        data = _f64(data)
        yf = np.asarray(y, dtype=np.float64)
        if indptr.ndim != 1 or indices.ndim != 1 or data.ndim != 1 or yf.ndim != 1 or indptr.size != yf.size + 1 or indices.size != data.size:
            raise ErrorInputParams("CSR arrays do not match: indptr has m + 1 entries, indices and data nnz each, y has m")
        m, k = yf.size, int(n_classes)
        bad = np.flatnonzero(~((yf >= 0) & (yf < max(k, 0)) & (yf == np.floor(yf))))
        if bad.size:
            raise ErrorInputParams(f"sparse multinomial: labels[{int(bad[0])}] = {yf[bad[0]]} is not an integer in [0, n_classes)")
        lab = np.ascontiguousarray(yf, dtype=np.int32)
        w = None if weights is None else _f64(weights)
        if w is not None and (w.ndim != 1 or w.size != m):
            raise ErrorInputParams(f"weights has {w.size} entries, a has {m} rows")
        # (an empty array's pointer may be null, which the library takes for a missing argument)
        ci = indices if indices.size else np.zeros(1, dtype=it)
        va = data if data.size else np.zeros(1)
        h = C.c_void_p()
        _check(A.lib().qn_sparse_multinomial_create(ctx.h, m, int(n), max(k, 0), data.size, indptr.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                                    it.itemsize, _dp(va), lab.ctypes.data_as(C.c_void_p), _dp(w) if w is not None else None, float(mu),
                                                    C.byref(h)))
        super().__init__(ctx, h, int(n) * k)
        self.m, self.n_features, self.n_classes = m, int(n), k

    @classmethod
    def from_scipy(cls, a, y, n_classes, mu, weights=None, ctx=None):
        """Any scipy sparse matrix (m x n): through .tocsr() with sorted indices and duplicates summed."""
        import scipy.sparse  # noqa: F401 -- only this method needs scipy
        a = a.tocsr().copy()
        a.sum_duplicates()
        a.sort_indices()
        return cls(a.indptr, a.indices, a.data, y, n_classes, mu, a.shape[1], weights=weights, ctx=ctx)

    def __call__(self, x):
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        if np.size(x) != self.n:
            raise ErrorInputParams(f"x has {np.size(x)} entries, the objective has {self.n}")
        return super().__call__(x)

    def _info(self):
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        nnz, lr, lc, nlr, nlc, kp = C.c_size_t(), C.c_int(), C.c_int(), C.c_size_t(), C.c_size_t(), C.c_int()
        _check(A.lib().qn_sparse_multinomial_info(self.h, C.byref(nnz), C.byref(lr), C.byref(lc), C.byref(nlr), C.byref(nlc), C.byref(kp)))
        return nnz.value, (lr.value, lc.value), nlr.value, nlc.value, kp.value

    @property
    def nnz(self):
        return self._info()[0]

    @property
    def lanes(self):
        """(entry lanes per row of the row pass over A, of the column pass over A')"""
        return self._info()[1]

    @property
    def n_long_rows(self):
        return self._info()[2]

    @property
    def n_long_cols(self):
        return self._info()[3]

    @property
    def kp(self):
        """The padded leading dimension of the feature-major copies: the next power of two of K up to 16, a multiple of 16 above."""
        return self._info()[4]

    def set_lanes(self, rows, cols):
        """Entry lanes that share one row of A (`rows`) and one row of A' (`cols`): 1, 2, 4, 8, 16, 32 or 64; 0: the choice made at creation.
        Another value may change the bits of f, g and H v."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        _check(A.lib().qn_sparse_multinomial_set_lanes(self.h, int(rows), int(cols)))

    def probabilities(self, x):
        """P at x, m x K: P[i, k] = p_ik (a masked row's are zeros).  One weights pass."""
        if not self.h:
            raise ErrorInputParams("the objective is closed")
        x = _f64(x)
        if x.size != self.n:
            raise ErrorInputParams(f"x has {x.size} entries, the objective has {self.n}")
        p = np.empty((self.m, self.n_classes))
        _check(A.lib().qn_sparse_multinomial_probabilities(self.h, _dp(x), _dp(p)))
        return p


class _SolverBase:
    METHOD = None

    def __init__(self, tol, x0, ctx=None):
        self.ctx = ctx or default_context()
        x0 = _f64(x0)
        self.n = x0.size
        self.h = C.c_void_p()
        _check(A.lib().qn_solver_create(self.ctx.h, self.METHOD, tol, _dp(x0), x0.size, C.byref(self.h)))
        self.memoize = None  # None: 1 for device objectives, 0 for host closures
        self._trace_cap = 0
        _live["solver"].add(self)

    @classmethod
    def new(cls, tol, x0, ctx=None):
        return cls(tol, x0, ctx)

    def reset(self, x0):
        """Back to the state right after `new(tol, x0)`."""
        x0 = _f64(x0)
        _check(A.lib().qn_solver_reset(self.h, _dp(x0)))

    def close(self):
        if getattr(self, "h", None):
            A.lib().qn_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def exact_state(self):
        """ExactQuadratic, of the last minimize: dict(curvature_passes, refreshes, last_t, last_curvature) -- refreshes: the accepted points (and
        forced re-evaluations of x) the objective itself evaluated, the first evaluation at x not counted."""
        passes, refreshes, t, c = C.c_size_t(), C.c_size_t(), C.c_double(), C.c_double()
        _check(A.lib().qn_solver_exact_state(self.h, C.byref(passes), C.byref(refreshes), C.byref(t), C.byref(c)))
        return dict(curvature_passes=passes.value, refreshes=refreshes.value, last_t=t.value, last_curvature=c.value)

    # ---- LineSearchSolver::minimize (ls_solver.rs:66-111) ----
    def minimize(self, line_search, oracle, max_iter_solver, max_iter_line_search, callback=None):
        L = A.lib()
        o = A.OracleStruct()
        keep = []
        if isinstance(oracle, Objective):
            o.kind = A.ORACLE_OBJECTIVE
            o.objective = oracle.h
            o.memoize = 1 if self.memoize is None else int(self.memoize)
        elif isinstance(oracle, DeviceClosure):
            o.kind, o.device_fn, o.device_user = A.ORACLE_DEVICE_FN, oracle.fn, oracle.user
            o.memoize = 0 if self.memoize is None else int(self.memoize)  # a closure: the reference's call sequence by default
        else:
            n = self.n
            err = []

            def tramp(_u, xp, nn, fp, gp):
                try:
                    x = np.ctypeslib.as_array(xp, shape=(nn,)).copy()
                    res = oracle(x)
                    f, g = (res.f(), res.g()) if isinstance(res, FuncEvalMultivariate) else res[:2]
                    fp[0] = float(f)
                    np.ctypeslib.as_array(gp, shape=(nn,))[:] = np.asarray(g, dtype=np.float64)
                    return 0
                except Exception as e:  # noqa: BLE001 -- a panicking closure aborts the run
                    err.append(e)
                    return 1
            def htramp(_u, xp, nn, hp):  # Newton: the Hessian part of the closure's FuncEval (newton/mod.rs:31-35)
                try:
                    x = np.ctypeslib.as_array(xp, shape=(nn,)).copy()
                    res = oracle(x)
                    hm = res.hessian() if isinstance(res, FuncEvalMultivariate) else (res[2] if len(res) > 2 else None)
                    if hm is None:
                        # projected_newton.rs:73, spn.rs:85 .expect(...): the library's own answer for an oracle without a Hessian
                        raise (RuntimeError if self.METHOD == A.NEWTON else ErrorInputParams)("Hessian not available in the oracle")
                    np.ctypeslib.as_array(hp, shape=(nn * nn,))[:] = np.asfortranarray(hm, dtype=np.float64).ravel(order="F")
                    return 0
                except Exception as e:  # noqa: BLE001
                    err.append(e)
                    return 1
            cfn = A.HOST_ORACLE_FN(tramp)
            keep.append(cfn)
            o.kind = A.ORACLE_HOST
            o.host_fn = C.cast(cfn, C.c_void_p)
            if self.METHOD in (A.NEWTON, A.PROJECTED_NEWTON, A.SPECTRAL_PROJECTED_NEWTON):
                hfn = A.HOST_HESSIAN_FN(htramp)
                keep.append(hfn)
                o.host_hessian_fn = C.cast(hfn, C.c_void_p)
            o.memoize = 0 if self.memoize is None else int(self.memoize)
        cb = None
        if callback is not None:
            cb = A.CALLBACK_FN(lambda _u, _s: callback(self))
            keep.append(cb)
        status = L.qn_minimize(self.h, C.byref(line_search.s), C.byref(o), max_iter_solver, max_iter_line_search,
                               C.cast(cb, C.c_void_p) if cb else None, None)
        if not isinstance(oracle, (Objective, DeviceClosure)) and err:
            raise err[0]
        _check(status)

    # ---- getters (derive_getters, bfgs.rs:3-12 ; LineSearchSolver::xk/k, bfgs.rs:52-63) ----
    def x(self):
        out = np.empty(self.n)
        _check(A.lib().qn_solver_get_x(self.h, _dp(out)))
        return out

    xk = x

    def set_x(self, x):
        x = _f64(x)
        _check(A.lib().qn_solver_set_x(self.h, _dp(x)))

    def direction(self):
        """the vector family: the direction of the last accepted iteration (inside the callback: d_k of the iteration just reported)"""
        out = np.empty(self.n)
        _check(A.lib().qn_solver_get_direction(self.h, _dp(out)))
        return out

    def gradient(self):
        """the vector family: the gradient of the evaluation held at the current x (inside the callback, memoised: g_{k+1}); refused when none is"""
        out = np.empty(self.n)
        _check(A.lib().qn_solver_get_gradient(self.h, _dp(out)))
        return out

    def k(self):
        return A.lib().qn_solver_k(self.h)

    def set_k(self, k):  # k_mut(), bfgs.rs:58-63
        _check(A.lib().qn_solver_set_k(self.h, int(k)))

    def identity(self):  # derive_getters on bfgs.rs:9 `identity: DMatrix<Floating>`; the GPU solver keeps no copy of it
        return np.eye(self.n)

    def tol(self):
        return A.lib().qn_solver_tol(self.h)

    def _opt(self, fn):
        v, some = C.c_double(), C.c_int()
        _check(fn(self.h, C.byref(v), C.byref(some)))
        return v.value if some.value else None

    def s_norm(self):
        return self._opt(A.lib().qn_solver_s_norm)

    def y_norm(self):
        return self._opt(A.lib().qn_solver_y_norm)

    def next_iterate_too_close(self):
        v = C.c_int()
        _check(A.lib().qn_solver_next_iterate_too_close(self.h, C.byref(v)))
        return bool(v.value)

    def gradient_next_iterate_too_close(self):
        v = C.c_int()
        _check(A.lib().qn_solver_gradient_next_iterate_too_close(self.h, C.byref(v)))
        return bool(v.value)

    def has_converged(self, eval_x_k):
        """bfgs.rs:64-76 evaluated on a host FuncEval (used by the reference's tests after minimize)."""
        if self.next_iterate_too_close() or self.gradient_next_iterate_too_close():
            return True
        g = eval_x_k.g() if isinstance(eval_x_k, FuncEvalMultivariate) else eval_x_k[1]
        return float(np.sqrt(np.dot(g, g))) < self.tol()

    def approx_inv_hessian(self, all_ranks=True):
        out = np.zeros((self.n, self.n), order="F")
        _check(A.lib().qn_solver_get_inv_hessian(self.h, out.ctypes.data_as(A.dp), 1 if all_ranks else 0))
        return np.ascontiguousarray(out)

    def compute_direction(self, eval_x_k):
        """ComputeDirection::compute_direction (ls_solver.rs:3-8; bfgs.rs:42-49, dfp.rs:42-49, gradient_descent.rs:24-30)"""
        g = _f64(eval_x_k.g() if isinstance(eval_x_k, FuncEvalMultivariate) else eval_x_k[1])
        if g.size != self.n:
            raise ErrorInputParams("gradient has the wrong dimension")
        d = np.empty(self.n)
        _check(A.lib().qn_solver_compute_direction(self.h, g.ctypes.data_as(A.dp), d.ctypes.data_as(A.dp)))
        return d

    def secant_update(self, s, y):
        """the inverse-Hessian half of `update_next_iterate` (bfgs.rs:92-130, dfp.rs:92-118) on its own"""
        s, y = _f64(s), _f64(y)
        if s.size != self.n or y.size != self.n:
            raise ErrorInputParams("s / y have the wrong dimension")
        _check(A.lib().qn_solver_secant_update(self.h, s.ctypes.data_as(A.dp), y.ctypes.data_as(A.dp)))

    def set_approx_inv_hessian(self, h):
        a = np.asfortranarray(h, dtype=np.float64)
        _check(A.lib().qn_solver_set_inv_hessian(self.h, a.ctypes.data_as(A.dp)))

    # ---- instrumentation ----
    def set_trace(self, cap, with_x=False):
        self._trace_cap = cap
        self._trace_x = with_x
        _check(A.lib().qn_solver_set_trace(self.h, cap, 1 if with_x else 0))

    def trace(self):
        cap = self._trace_cap
        recs = (A.TraceRec * max(cap, 1))()
        ln = C.c_size_t()
        xs = np.zeros((max(cap, 1), self.n)) if getattr(self, "_trace_x", False) else None
        _check(A.lib().qn_solver_get_trace(self.h, recs, cap, C.byref(ln), _dp(xs) if xs is not None else None))
        out = [dict(f=r.f, gnorm=r.gnorm, t=r.t, s_norm=r.s_norm, y_norm=r.y_norm, n_evals=r.n_evals, ls_iters=r.ls_iters,
                    ls_cases=r.ls_cases, updated=r.updated) for r in recs[:ln.value]]
        return out, (xs[:ln.value] if xs is not None else None)

    def stats(self):
        st = A.Stats()
        _check(A.lib().qn_solver_get_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in A.Stats._fields_}

    def set_profiling(self, on):
        _check(A.lib().qn_solver_set_profiling(self.h, 1 if on else 0))

    def set_sync_mode(self, sync):
        _check(A.lib().qn_solver_set_sync_mode(self.h, int(sync)))

    def set_tiling(self, rows_per_block=0, col_splits=0):
        """tuning of the fused row kernels (rows per tile 2 / 4 / 8 / 16, column splits); diagnostics are named options: set_option"""
        _check(A.lib().qn_solver_set_tiling(self.h, rows_per_block, col_splits))

    def set_option(self, option, value=1):
        """qn_solver_set_option: `option` is a qn_option value (the OPT_* constants of this module) or its lower-case name without the prefix
        ("second_generation", "newton_pivoted_lu", ...); value != 0 switches the named thing on, 0 off."""
        if isinstance(option, str):
            option = OPTIONS[option]
        _check(A.lib().qn_solver_set_option(self.h, int(option), int(value)))

    def configure(self, what, value=0):
        """one entry point for parameter lists in tests and tools: configure(rows_per_block, col_splits) tunes, configure("option_name", v) sets a
        named option"""
        if isinstance(what, str):
            self.set_option(what, value)
        else:
            self.set_tiling(what, value)


class BFGS(_SolverBase):
    """quasi_newton/bfgs.rs"""
    METHOD = A.BFGS


class DFP(_SolverBase):
    """quasi_newton/dfp.rs"""
    METHOD = A.DFP


class Broyden(_SolverBase):
    """quasi_newton/broyden.rs: H += ((s - H y) s') H / (s . y) as written -- H is not symmetric after the first update"""
    METHOD = A.BROYDEN


class GradientDescent(_SolverBase):
    """steepest_descent/gradient_descent.rs (config-1 plumbing)"""
    METHOD = A.GRADIENT_DESCENT

    def has_converged(self, eval_x_k):
        g = eval_x_k.g() if isinstance(eval_x_k, FuncEvalMultivariate) else eval_x_k[1]
        return float(np.max(np.abs(g))) < self.tol()


class CoordinateDescent(GradientDescent):
    """steepest_descent/coordinate_descent.rs, as written: d = -e_p with p the first index of the largest |g_i| -- whatever the sign of g_p
    (`-max_value.signum()` of a magnitude, coordinate_descent.rs:43)."""
    METHOD = A.COORDINATE_DESCENT

    def grad_tol(self):
        return self.tol()


class PnormDescent(GradientDescent):
    """steepest_descent/pnorm_descent.rs: d = (-inverse_p) * g with a dense n x n matrix that never changes (any matrix: neither symmetry nor
    definiteness is tested).  One read-only stream of the matrix per iteration on the GPU; `reset` keeps it."""
    METHOD = A.PNORM_DESCENT

    def __init__(self, grad_tol, x0, inverse_p, ctx=None):
        super().__init__(grad_tol, x0, ctx)
        if inverse_p is not None:  # (None: qn_solver_create alone; minimize then answers ErrorInputParams until set_inverse_p)
            self.set_inverse_p(inverse_p)

    def set_inverse_p(self, inverse_p):
        p = np.asfortranarray(inverse_p, dtype=np.float64)
        if p.shape != (self.n, self.n):
            raise ErrorInputParams("inverse_p must be n x n")
        _check(A.lib().qn_solver_set_inverse_p(self.h, p.ctypes.data_as(A.dp)))

    @classmethod
    def new(cls, grad_tol, x0, inverse_p, ctx=None):
        return cls(grad_tol, x0, inverse_p, ctx)

    def grad_tol(self):
        return self.tol()

    def inverse_p(self):
        out = np.zeros((self.n, self.n), order="F")
        _check(A.lib().qn_solver_get_inverse_p(self.h, out.ctypes.data_as(A.dp)))
        return np.ascontiguousarray(out)


class _BoundedBase(_SolverBase):
    """bfgs_b.rs / dfp_b.rs / sr1_b.rs: `new(tol, x0, lower_bound, upper_bound)`; x0 is projected, directions are P(x - Hg) - x."""

    def __init__(self, tol, x0, lower_bound, upper_bound, ctx=None):
        super().__init__(tol, x0, ctx)
        self._lb, self._ub = _f64(lower_bound), _f64(upper_bound)
        _check(A.lib().qn_solver_set_bounds(self.h, _dp(self._lb), _dp(self._ub)))

    @classmethod
    def new(cls, tol, x0, lower_bound, upper_bound, ctx=None):
        return cls(tol, x0, lower_bound, upper_bound, ctx)

    def lower_bound(self):
        return self._lb

    def upper_bound(self):
        return self._ub

    def projected_gradient(self, eval_x_k):  # ls_solver.rs:121-133
        g = np.array(eval_x_k.g() if isinstance(eval_x_k, FuncEvalMultivariate) else eval_x_k[1], dtype=np.float64)
        x = self.x()
        g[((x == self._lb) & (g > 0)) | ((x == self._ub) & (g < 0))] = 0.0
        return g


class BFGSB(_BoundedBase):
    METHOD = A.BFGS


class DFPB(_BoundedBase):
    METHOD = A.DFP


class SR1B(_BoundedBase):
    METHOD = A.SR1


class BroydenB(_BoundedBase):
    """quasi_newton/broyden_b.rs"""
    METHOD = A.BROYDEN


class _ProjectedBase(_BoundedBase):
    """The first-order family (steepest_descent/spg.rs, projected_gradient_descent.rs): O(n) state, no inverse Hessian."""

    def grad_tol(self):
        return self.tol()

    def approx_inv_hessian(self, all_ranks=True):  # there is none: the library says so (no n x n buffer is made to find out)
        _check(A.lib().qn_solver_get_inv_hessian(self.h, None, 0))

    def set_approx_inv_hessian(self, h):
        _check(A.lib().qn_solver_set_inv_hessian(self.h, None))

    def has_converged(self, eval_x_k):  # spg.rs:89-92, projected_gradient_descent.rs:76-83
        return float(np.max(np.abs(self.projected_gradient(eval_x_k)))) < self.tol()


class ProjectedGradientDescent(_ProjectedBase):
    """steepest_descent/projected_gradient_descent.rs: `new(grad_tol, x0, lower_bound, upper_bound)`; d = P(x - g) - x."""
    METHOD = A.PROJECTED_GRADIENT


class SpectralProjectedGradient(_ProjectedBase):
    """steepest_descent/spg.rs: `new(grad_tol, x0, oracle, lower_bound, upper_bound)`; d = P(x - lambda g) - x with the safeguarded
    Barzilai-Borwein scalar.  As in the reference the constructor calls the oracle once, for lambda0 (spg.rs:40-46)."""
    METHOD = A.SPG

    def __init__(self, grad_tol, x0, oracle, lower_bound, upper_bound, ctx=None, memoize=None):
        super().__init__(grad_tol, x0, lower_bound, upper_bound, ctx)
        self.memoize = memoize
        try:  # a call with no iterations: the constructor's evaluation only
            self.minimize(GLLQuadratic(1e-4, 1), oracle, 0, 0)
        except MaxIterReached:
            pass

    @classmethod
    def new(cls, grad_tol, x0, oracle, lower_bound, upper_bound, ctx=None, memoize=None):
        return cls(grad_tol, x0, oracle, lower_bound, upper_bound, ctx, memoize)

    def with_lambdas(self, lambda_min, lambda_max):  # spg.rs:23-27
        _check(A.lib().qn_solver_set_spg_lambdas(self.h, float(lambda_min), float(lambda_max)))
        self._lmin, self._lmax = float(lambda_min), float(lambda_max)
        return self

    def lambda_(self):
        return self._opt(A.lib().qn_solver_spg_lambda)

    # (the ABI has a setter for the two bounds and no getter: these return what this object last set, or spg.rs:36-37's defaults)
    def lambda_min(self):
        return getattr(self, "_lmin", 1e-3)

    def lambda_max(self):
        return getattr(self, "_lmax", 1e3)


class SpectralProximalGradient(_SolverBase):
    """Spectral proximal gradient (SpaRSA): min f(x) + sum_j l1_j |x_j| over lb <= x <= ub.  SPG with the projection replaced by the proximal map
    of lambda l1 |.| plus the box: d = clip(soft(x - lambda g, lambda l1)) - x, the search (GLLQuadratic or BackTracking) on the composite value
    with Tseng and Yun's decrease g.d + h(x + d) - h(x).  `l1`: one scalar or one value per entry, >= 0 and finite.  The constructor evaluates once,
    for lambda0, as SpectralProjectedGradient's does.  Entries the prox sets to zero are exactly 0.0 in x()."""
    METHOD = A.SPECTRAL_PROXIMAL_GRADIENT

    def __init__(self, tol, x0, oracle, l1, lower_bound=None, upper_bound=None, ctx=None, memoize=None):
        super().__init__(tol, x0, ctx)
        self._lb = self._ub = None
        if lower_bound is not None or upper_bound is not None:
            self._lb = _f64(np.full(self.n, -np.inf) if lower_bound is None else lower_bound)
            self._ub = _f64(np.full(self.n, np.inf) if upper_bound is None else upper_bound)
            _check(A.lib().qn_solver_set_bounds(self.h, _dp(self._lb), _dp(self._ub)))
        self.set_l1(l1)
        self.memoize = memoize
        try:  # a call with no iterations: the constructor's evaluation only
            self.minimize(GLLQuadratic(1e-4, 1), oracle, 0, 0)
        except MaxIterReached:
            pass

    @classmethod
    def new(cls, tol, x0, oracle, l1, lower_bound=None, upper_bound=None, ctx=None, memoize=None):
        return cls(tol, x0, oracle, l1, lower_bound, upper_bound, ctx, memoize)

    def set_l1(self, v):
        """a scalar or n entries; between two minimize calls: the ring is cleared, lambda, x and the memoised evaluation are kept"""
        if np.ndim(v) == 0:
            _check(A.lib().qn_solver_set_l1(self.h, None, float(v)))
        else:
            v = _f64(v)
            if v.size != self.n:
                raise ErrorInputParams("l1 has the wrong dimension")
            _check(A.lib().qn_solver_set_l1(self.h, _dp(v), 0.0))

    @property
    def l1(self):
        out = np.empty(self.n)
        _check(A.lib().qn_solver_get_l1(self.h, _dp(out)))
        return out

    with_lambdas = SpectralProjectedGradient.with_lambdas
    lambda_ = SpectralProjectedGradient.lambda_
    lambda_min = SpectralProjectedGradient.lambda_min
    lambda_max = SpectralProjectedGradient.lambda_max

    def grad_tol(self):
        return self.tol()

    def lower_bound(self):
        return self._lb

    def upper_bound(self):
        return self._ub

    def penalty(self):
        """h at x()"""
        return float(np.dot(self.l1, np.abs(self.x())))

    def composite(self, eval_x_k):
        """F = f + h at x(), from an evaluation of the smooth part there"""
        f = eval_x_k.f() if isinstance(eval_x_k, FuncEvalMultivariate) else eval_x_k[0]
        return float(f) + self.penalty()

    def nonzeros(self):
        return int(np.count_nonzero(self.x()))

    def measure(self, eval_x_k):
        """per entry, the element of least magnitude of the subdifferential of F at x(), opened towards the side a bound blocks"""
        g = np.asarray(eval_x_k.g() if isinstance(eval_x_k, FuncEvalMultivariate) else eval_x_k[1], dtype=np.float64)
        x, l1 = self.x(), self.l1
        lo = np.where(x > 0.0, g + l1, g - l1)
        hi = np.where(x < 0.0, g - l1, g + l1)
        if self._lb is not None:
            lo = np.where(x == self._lb, -np.inf, lo)
            hi = np.where(x == self._ub, np.inf, hi)
        return np.where(lo > 0.0, lo, np.where(hi < 0.0, hi, 0.0))

    def has_converged(self, eval_x_k):
        return float(np.max(np.abs(self.measure(eval_x_k)))) < self.tol()

    def approx_inv_hessian(self, all_ranks=True):  # there is none
        _check(A.lib().qn_solver_get_inv_hessian(self.h, None, 0))

    def set_approx_inv_hessian(self, h):
        _check(A.lib().qn_solver_set_inv_hessian(self.h, None))


class ProjectedNewton(_ProjectedBase):
    """newton/projected_newton.rs: `new(grad_tol, x0, lower_bound, upper_bound)`; d = P(x - H^-1 g) - x with H^-1 g from one Cholesky
    factorisation (the lower triangle of the Hessian) and one solve on the GPU.  The oracle is a `Quadratic` (its matrix is the Hessian) or
    a closure returning `FuncEvalMultivariate(f, g).with_hessian(h)`; anything else has no Hessian here: ErrorInputParams."""
    METHOD = A.PROJECTED_NEWTON

    def has_converged(self, eval_x_k):  # projected_newton.rs:95-110: s_norm, then y_norm, then the projected gradient
        if self.next_iterate_too_close() or self.gradient_next_iterate_too_close():
            return True
        return float(np.max(np.abs(self.projected_gradient(eval_x_k)))) < self.tol()

    def newton_factorisations(self):
        v = C.c_size_t()
        _check(A.lib().qn_solver_newton_factorisations(self.h, C.byref(v)))
        return v.value


class SpectralProjectedNewton(SpectralProjectedGradient):
    """newton/spn.rs: `new(grad_tol, x0, oracle, lower_bound, upper_bound)`; d = P(x - lambda H^-1 g) - x, lambda built and updated exactly as
    in SpectralProjectedGradient (the constructor calls the oracle once, for lambda0: spn.rs:40-46; no Hessian is needed there)."""
    METHOD = A.SPECTRAL_PROJECTED_NEWTON

    newton_factorisations = ProjectedNewton.newton_factorisations


class ProjectedLBFGS(_ProjectedBase):
    """Limited-memory BFGS in a box: `new(tol, x0, lower_bound, upper_bound, m=5)`; d = P(x - H_k g) - x with H_k g from the last m pairs (s, y)
    in the compact form (two streams of the memory and one small solve per iteration on the GPU).  NOT the reference's `Lbfgsb` (the Fortran
    L-BFGS-B: no generalised Cauchy point, no subspace minimisation here): the bounded variant follows BFGSB's convention (bfgs_b.rs:72-75), and
    with an active box its direction is no more guaranteed to descend than BFGSB's."""
    METHOD = A.LBFGS

    def __init__(self, tol, x0, lower_bound, upper_bound, m=5, ctx=None, memoize=None):
        super().__init__(tol, x0, lower_bound, upper_bound, ctx)
        self.memoize = memoize
        if m != 5:
            self.set_memory(m)

    @classmethod
    def new(cls, tol, x0, lower_bound, upper_bound, m=5, ctx=None, memoize=None):
        return cls(tol, x0, lower_bound, upper_bound, m, ctx, memoize)

    def set_memory(self, m):
        """qn_solver_set_lbfgs_memory: 1 <= m <= 32; the stored pairs are dropped"""
        if not 0 <= int(m) < 2 ** 63:
            raise ErrorInputParams("L-BFGS: the memory m must be 1 .. 32")
        _check(A.lib().qn_solver_set_lbfgs_memory(self.h, int(m)))

    def _lbfgs_state(self):
        m, stored, resets, gamma = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_double()
        _check(A.lib().qn_solver_lbfgs_state(self.h, C.byref(m), C.byref(stored), C.byref(gamma), C.byref(resets)))
        return m.value, stored.value, gamma.value, resets.value

    @property
    def memory(self):
        return self._lbfgs_state()[0]

    def stored_pairs(self):
        return self._lbfgs_state()[1]

    def gamma(self):
        return self._lbfgs_state()[2]

    def resets(self):
        return self._lbfgs_state()[3]


class LBFGS(ProjectedLBFGS):
    """Limited-memory BFGS: `new(tol, x0, m=5)`; d = -H_k g.  The same solver with the box left at (-inf, +inf)."""

    def __init__(self, tol, x0, m=5, ctx=None, memoize=None):
        n = _f64(x0).size
        super().__init__(tol, x0, np.full(n, -np.inf), np.full(n, np.inf), m, ctx, memoize)

    @classmethod
    def new(cls, tol, x0, m=5, ctx=None, memoize=None):
        return cls(tol, x0, m, ctx, memoize)


class OWLQN(_SolverBase):
    """Orthant-wise limited-memory quasi-Newton (Andrew and Gao 2007): min f(x) + sum_j l1_j |x_j|, unbounded.  `new(tol, x0, l1, m=5)`; L-BFGS's
    memory and compact-form direction applied to the pseudo-gradient v, the direction aligned with -v, every trial point projected onto the orthant
    of x (of -v where x is 0), `BackTracking` on the composite value.  `l1`: one scalar or one value per entry, >= 0 and finite; an entry with
    l1 == 0 is smooth.  Entries the projection switches off are exactly 0.0 in x().  The pairs are differences of the smooth gradient: `set_l1`
    between two minimize calls keeps them, x and the memoised evaluation (the regularisation path)."""
    METHOD = A.OWLQN

    def __init__(self, tol, x0, l1, m=5, ctx=None, memoize=None):
        super().__init__(tol, x0, ctx)
        self.memoize = memoize
        self.set_l1(l1)
        if m != 5:
            self.set_memory(m)

    @classmethod
    def new(cls, tol, x0, l1, m=5, ctx=None, memoize=None):
        return cls(tol, x0, l1, m, ctx, memoize)

    set_l1 = SpectralProximalGradient.set_l1
    l1 = SpectralProximalGradient.l1
    penalty = SpectralProximalGradient.penalty
    composite = SpectralProximalGradient.composite
    nonzeros = SpectralProximalGradient.nonzeros
    approx_inv_hessian = SpectralProximalGradient.approx_inv_hessian
    set_approx_inv_hessian = SpectralProximalGradient.set_approx_inv_hessian
    set_memory = ProjectedLBFGS.set_memory
    _lbfgs_state = ProjectedLBFGS._lbfgs_state
    memory = ProjectedLBFGS.memory
    stored_pairs = ProjectedLBFGS.stored_pairs
    gamma = ProjectedLBFGS.gamma
    resets = ProjectedLBFGS.resets

    def grad_tol(self):
        return self.tol()

    def pseudo_gradient(self):
        """v of the last loop top (inside the callback: v_k of the iteration just reported)"""
        out = np.empty(self.n)
        _check(A.lib().qn_solver_get_pseudo_gradient(self.h, _dp(out)))
        return out

    def measure(self, eval_x_k):
        """the pseudo-gradient at x() from an evaluation of the smooth part there: SpectralProximalGradient's measure without a box"""
        g = np.asarray(eval_x_k.g() if isinstance(eval_x_k, FuncEvalMultivariate) else eval_x_k[1], dtype=np.float64)
        x, l1 = self.x(), self.l1
        lo = np.where(x > 0.0, g + l1, g - l1)
        hi = np.where(x < 0.0, g - l1, g + l1)
        return np.where(lo > 0.0, lo, np.where(hi < 0.0, hi, 0.0))

    def has_converged(self, eval_x_k):
        return float(np.max(np.abs(self.measure(eval_x_k)))) < self.tol()


class NonlinearCG(_SolverBase):
    """Nonlinear conjugate gradient: `new(tol, x0, variant="pr+", powell_nu=0.2, restart_every=0)`; d+ = beta d - g+ with beta by the variant --
    "fr" (Fletcher-Reeves), "pr+" (Polak-Ribiere+), "hs+" (Hestenes-Stiefel+), "dy" (Dai-Yuan), "hz" (Hager-Zhang) -- and restarts d = -g by
    Powell's test |g+.g| >= powell_nu g+.g+ (inf: off), every `restart_every` iterations (0: never), and whenever beta d - g+ would not descend.
    One extra vector of state.  UNBOUNDED ONLY; line searches: StrongWolfe (what "fr", "dy" and "hs+" assume) and BackTracking."""
    METHOD = A.NONLINEAR_CG
    VARIANTS = {"fr": A.CG_FR, "pr+": A.CG_PR_PLUS, "hs+": A.CG_HS_PLUS, "dy": A.CG_DY, "hz": A.CG_HZ}

    def __init__(self, tol, x0, variant="pr+", powell_nu=0.2, restart_every=0, memoize=None, ctx=None):
        super().__init__(tol, x0, ctx)
        self.memoize = memoize
        if (variant, powell_nu, restart_every) != ("pr+", 0.2, 0):
            self.set_cg(variant, powell_nu, restart_every)

    @classmethod
    def new(cls, tol, x0, variant="pr+", powell_nu=0.2, restart_every=0, memoize=None, ctx=None):
        return cls(tol, x0, variant, powell_nu, restart_every, memoize, ctx)

    def set_cg(self, variant="pr+", powell_nu=0.2, restart_every=0):
        """qn_solver_set_cg: the stored direction is dropped (the next direction is -g)"""
        code = self.VARIANTS.get(variant, variant)
        if not isinstance(code, int) or isinstance(code, bool):
            raise ErrorInputParams('NonlinearCG: unknown variant (one of "fr", "pr+", "hs+", "dy", "hz")')
        if not 0 <= int(restart_every) < 2 ** 63:
            raise ErrorInputParams("NonlinearCG: restart_every must not be negative")
        _check(A.lib().qn_solver_set_cg(self.h, code, float(powell_nu), int(restart_every)))

    def _cg_state(self):
        variant, beta, restarts, since = C.c_int(), C.c_double(), C.c_size_t(), C.c_size_t()
        _check(A.lib().qn_solver_cg_state(self.h, C.byref(variant), C.byref(beta), C.byref(restarts), C.byref(since)))
        return variant.value, beta.value, restarts.value, since.value

    @property
    def variant(self):
        code = self._cg_state()[0]
        return next(k for k, v in self.VARIANTS.items() if v == code)

    def beta(self):
        """of the last accepted iteration: what the next direction is made with (0 before the first, and after a restart)"""
        return self._cg_state()[1]

    def restarts(self):
        return self._cg_state()[2]

    def since_restart(self):
        return self._cg_state()[3]

    def grad_tol(self):
        return self.tol()


class NewtonCG(_SolverBase):
    """Truncated Newton: `new(tol, x0, eta_max=0.5, max_inner=0, chunk=8, preconditioner="none")`; Newton's direction from a few conjugate-gradient steps on H z = g,
    each costing one Hessian-vector product of the device LogSumExp or Logistic objective (one stream of A, never a matrix).  The inner loop ends once
    ||r|| <= min(eta_max, sqrt(||g||)) ||g||, after max_inner steps (0: min(n, 100)) or on curvature that is not positive; `chunk` inner steps
    are enqueued per batch (it never changes a bit).  UNBOUNDED ONLY; objective: LogSumExp or Logistic with n_pad <= 16384, or SparseLogistic (any n); line searches: BackTracking and
    StrongWolfe, first trial t = 1.  Closures, quadratics, other searches: ErrorInputParams.  preconditioner="jacobi" (opt-in, see `set_preconditioner`)
    divides the inner loop's residual by diag H(x_k): fewer inner steps where the columns of A differ in scale by orders of magnitude, nothing gained
    where they do not."""
    METHOD = A.NEWTON_CG
    PRECONDITIONERS = {"none": A.PRECOND_NONE, "jacobi": A.PRECOND_JACOBI}

    def __init__(self, tol, x0, eta_max=0.5, max_inner=0, chunk=8, memoize=None, ctx=None, preconditioner="none"):
        super().__init__(tol, x0, ctx)
        self.memoize = memoize
        if (eta_max, max_inner, chunk) != (0.5, 0, 8):
            self.set_newton_cg(eta_max, max_inner, chunk)
        if preconditioner != "none":
            self.set_preconditioner(preconditioner)

    @classmethod
    def new(cls, tol, x0, eta_max=0.5, max_inner=0, chunk=8, memoize=None, ctx=None, preconditioner="none"):
        return cls(tol, x0, eta_max, max_inner, chunk, memoize, ctx, preconditioner)

    def set_preconditioner(self, kind):
        """"none" (the default: plain conjugate gradients) or "jacobi": the inner loop preconditioned by diag H(x_k), one more pass of A per outer
        iteration (`Objective.hess_diag_at`'s launches).  It pays where the columns of A differ in scale by orders of magnitude (2 to 4 times fewer
        inner steps); on well-scaled columns the extra pass buys nothing, and with m < n and a small mu it can lose.  LogSumExp, Logistic and
        SparseLogistic only: another objective is refused at minimize."""
        if kind not in self.PRECONDITIONERS:
            raise ErrorInputParams('NewtonCG: preconditioner is "none" or "jacobi"')
        _check(A.lib().qn_solver_set_newton_cg_preconditioner(self.h, self.PRECONDITIONERS[kind]))

    def _pc_state(self):
        kind, passes, floored = C.c_int(), C.c_size_t(), C.c_size_t()
        _check(A.lib().qn_solver_newton_cg_precond_state(self.h, C.byref(kind), C.byref(passes), C.byref(floored)))
        return kind.value, passes.value, floored.value

    @property
    def preconditioner(self):
        return {v: k for k, v in self.PRECONDITIONERS.items()}[self._pc_state()[0]]

    def diag_passes(self):
        """directions of the last minimize that started with a diagonal pass (0 without a preconditioner)"""
        return self._pc_state()[1]

    def preconditioner_diag(self):
        """(M, 1 / M) of the last diagonal pass: diag H(x) at the point of the run's last loop top and what rule 2' made of it, n entries each"""
        m, minv = np.empty(self.n), np.empty(self.n)
        _check(A.lib().qn_solver_newton_cg_precond_diag(self.h, _dp(m), _dp(minv)))
        return m, minv

    def diag_floored(self):
        """entries of the last direction's 1 / M that were set to 1 because M_j was not positive and finite"""
        return self._pc_state()[2]

    def set_newton_cg(self, eta_max=0.5, max_inner=0, chunk=8):
        if not 0 <= int(max_inner) < 2 ** 63 or not 0 <= int(chunk) < 2 ** 63:
            raise ErrorInputParams("NewtonCG: max_inner and chunk must not be negative")
        _check(A.lib().qn_solver_set_newton_cg(self.h, float(eta_max), int(max_inner), int(chunk)))

    def _tn_state(self):
        v = [C.c_size_t() for _ in range(5)]
        _check(A.lib().qn_solver_newton_cg_state(self.h, *[C.byref(x) for x in v]))
        return [x.value for x in v]

    def inner_iterations(self):
        """(inner steps of the last direction, of all directions of the last minimize)"""
        s = self._tn_state()
        return s[0], s[1]

    def hv_passes(self):
        return self._tn_state()[2]

    def negative_curvature(self):
        return self._tn_state()[3]

    def fallbacks(self):
        return self._tn_state()[4]

    def grad_tol(self):
        return self.tol()


class Newton(_SolverBase):
    """newton/mod.rs: direction from a dense factorisation of the Hessian on the GPU."""
    METHOD = A.NEWTON

    def decrement_squared(self):
        return self._opt(A.lib().qn_solver_decrement_squared)

    def has_converged(self, eval_x_k=None):  # newton/mod.rs:64-69
        d = self.decrement_squared()
        return d is not None and d * 0.5 < self.tol()


# ---- kernel-level FFI helpers (tests of the individual primitives) ----
class DeviceBuffer:
    def __init__(self, ctx, host_array):
        a = _f64(host_array)
        self.ctx, self.shape, self.nbytes = ctx, a.shape, a.nbytes
        self.p = C.c_void_p()
        _check(A.lib().qn_dev_alloc(ctx.h, max(a.nbytes, 8), C.byref(self.p)))
        if a.nbytes:
            _check(A.lib().qn_h2d(ctx.h, self.p, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def get(self):
        out = np.empty(self.shape)
        if self.nbytes:
            _check(A.lib().qn_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.p, self.nbytes))
        return out

    def free(self):
        if self.p:
            A.lib().qn_dev_free(self.ctx.h, self.p)
            self.p = None


def gemv(ctx, a_dev, ld, nrows, ncols, x_dev, y_dev):
    _check(A.lib().qn_gemv(ctx.h, a_dev.p, ld, nrows, ncols, x_dev.p, y_dev.p))


def rank2_update(ctx, h_dev, ld, row0, nrows, n, s_dev, u_dev, c_ss, c_su, c_uu):
    _check(A.lib().qn_rank2_update(ctx.h, h_dev.p, ld, row0, nrows, n, s_dev.p, u_dev.p, c_ss, c_su, c_uu))


def axpy(ctx, n, x_dev, t, d_dev, out_dev):
    _check(A.lib().qn_axpy(ctx.h, n, x_dev.p, t, d_dev.p, out_dev.p))


def dot(ctx, n, a_dev, b_dev):
    v = C.c_double()
    _check(A.lib().qn_dot(ctx.h, n, a_dev.p, b_dev.p, C.byref(v)))
    return v.value


def nrm2(ctx, n, a_dev):
    v = C.c_double()
    _check(A.lib().qn_nrm2(ctx.h, n, a_dev.p, C.byref(v)))
    return v.value
