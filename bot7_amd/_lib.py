"""ctypes binding of libbot7hip.so (include/bot7hip.h) and a thin ``Context`` wrapper.

No fallbacks: if the shared library is missing or no gfx950 device is present, the first use raises
``Bot7HipError``.  Nothing in this package computes on the CPU.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BOT7HIP_LIB: the same override the LuaJIT binding honours (lua/bot7hip_ffi.lua); diagnostic builds use it (tools/)
_SO = os.environ.get("BOT7HIP_LIB") or os.path.join(_HERE, "libbot7hip.so")

B7_OK = 0
ERR_NAMES = {-1: "B7_ERR_INVALID", -2: "B7_ERR_HIP", -3: "B7_ERR_NOMEM", -4: "B7_ERR_STATE",
             -5: "B7_ERR_UNSUPPORTED", -6: "B7_ERR_RANGE", -7: "B7_ERR_COMM"}

# Every symbol include/bot7hip.h declares (tests check the library exports each of them).
SYMBOLS = [
    "b7_abi_version", "b7_create", "b7_destroy", "b7_last_error", "b7_device_info", "b7_sync", "b7_set_workspace",
    "b7_sobol_direction_numbers", "b7_grid_sobol", "b7_grid_random", "b7_grid_upload", "b7_grid_download", "b7_grid_shape", "b7_grid_remove", "b7_grid_remove_rows",
    "b7_grid_colrange", "b7_grid_apply_onesided", "b7_grid_random_torch", "b7_torch_rand",
    "b7_grid_trust_region", "b7_tr_box", "b7_tr_init", "b7_tr_update",
    "b7_gp_default_opts", "b7_gp_set_opts", "b7_gp_set_kernel", "b7_gp_fit", "b7_gp_set_data", "b7_gp_fit_hyp", "b7_gp_predict_hyp", "b7_gp_nll_batch", "b7_gp_slice_sample", "b7_gp_slice_trace_enable", "b7_gp_slice_trace", "b7_chol", "b7_gp_predict", "b7_gp_predict_at", "b7_gp_fantasize", "b7_gp_append", "b7_gp_download",
    "b7_blr_basis", "b7_blr_features", "b7_blr_fit", "b7_blr_fit_x", "b7_blr_predict", "b7_score_reset", "b7_score_ei", "b7_score_logei", "b7_score_mes", "b7_mes_set_levels", "b7_mes_last_ystar", "b7_mes_ystar", "b7_mes_compute", "b7_score_cb", "b7_score_finish",
    "b7_comm_pick_winner", "b7_comm_unique_id", "b7_comm_init", "b7_comm_info", "b7_comm_destroy", "b7_comm_allreduce_f64", "b7_score_finish_global", "b7_eval_nominate", "b7_eval_nominate_batch", "b7_blr_eval_nominate", "b7_blr_eval_nominate_marg",
    "b7_ts_nominate", "b7_ts_last_paths", "b7_ts_last_draws", "b7_rff_compute",
    "b7_ts_nominate_refine", "b7_ts_refine_last", "b7_ts_refine_trace_enable", "b7_ts_refine_trace", "b7_ts_path_grad_at",
    "b7_blr_ts_nominate", "b7_blr_ts_last_draws", "b7_blr_paths_compute",
    "b7_kg_nominate", "b7_kg_trace_enable", "b7_kg_last", "b7_kg_compute",
    "b7_eval_posterior", "b7_posterior_get", "b7_pareto_front2", "b7_hypervolume2", "b7_ehvi_compute", "b7_ehvi_nominate",
    "b7_pareto_front3", "b7_nondominated_boxes3", "b7_hypervolume3", "b7_ehvi3_compute", "b7_ehvi3_nominate",
    "b7_logehvi_compute", "b7_logehvi_nominate", "b7_logehvi3_compute", "b7_logehvi3_nominate",
    "b7_ts_paths", "b7_ts_hvi_nominate", "b7_ts_hvi3_nominate", "b7_hvi_compute",
    "b7_ts_feas_nominate", "b7_ts_feas_compute",
    "b7_refine_default_opts", "b7_eval_nominate_refine", "b7_refine_last", "b7_refine_shape", "b7_refine_trace_enable", "b7_refine_trace", "b7_gp_grad_at", "b7_score_grad_compute",
    "b7_nominate_commit", "b7_shard_commit_rule", "b7_exchange_info",
    "b7_group_create", "b7_group_destroy", "b7_group_last_error", "b7_group_info", "b7_group_ctx", "b7_group_set_workspace", "b7_group_gp_set_opts", "b7_group_gp_set_kernel",
    "b7_group_grid_sobol", "b7_group_grid_random", "b7_group_grid_onesided", "b7_group_grid_upload", "b7_group_grid_shape", "b7_group_grid_download",
    "b7_group_grid_remove_rows", "b7_group_gp_set_data", "b7_group_eval_nominate", "b7_group_nominate_commit",
    "b7_ei_compute", "b7_cb_compute", "b7_logei_compute", "b7_argmax",
    "b7_score_logpi", "b7_logpi_compute", "b7_feas_reset", "b7_feas_add", "b7_feas_add_acc", "b7_feas_get", "b7_feas_nominate", "b7_eval_nominate_feasible",
    "b7_clf_nll_batch", "b7_clf_fit_hyp", "b7_clf_mode_get", "b7_clf_eval_logfeas", "b7_probit_compute",
    "b7_gp_fit_hyp_grad", "b7_gp_nll_grad", "b7_lbfgsb_default_opts", "b7_lbfgsb_minimize", "b7_gp_fit_map", "b7_gp_fit_map_trace_enable", "b7_gp_fit_map_trace",
    "b7_timer_start", "b7_timer_stop", "b7_timer_ms", "b7_profile_enable", "b7_profile_reset", "b7_profile_get", "b7_persist_fallbacks",
]


KG_MAX_POINTS = 16  # B7_KG_MAX_POINTS
EHVI_PMAX, EHVI_SMAX, EHVI_SREG = 256, 32, 10  # B7_EHVI_PMAX (front points), B7_EHVI_SMAX (hyper samples per objective), B7_EHVI_SREG (of them in registers)
EHVI3_PMAX = 256  # B7_EHVI3_PMAX (front points of three objectives)
TS_FEAS_CMAX = 8  # B7_TS_FEAS_CMAX (constraints of a constrained Thompson nomination)
TS_FEAS_THREADS, TS_FEAS_BLOCKS_MAX = 256, 1024  # csrc/ts_feas.hip's launch shape: above their product rows the grid-stride loop wraps


class Bot7HipError(RuntimeError):
    def __init__(self, code, message):
        self.code = code
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "B7_ERR"), code, message))


class Hyp(C.Structure):
    _fields_ = [("lenscale_sq", C.POINTER(C.c_double)), ("amp", C.c_double), ("noise", C.c_double),
                ("mean", C.c_double)]


class TrState(C.Structure):   # b7_tr_state
    _fields_ = [("length", C.c_double), ("length_init", C.c_double), ("length_min", C.c_double), ("length_max", C.c_double),
                ("best", C.c_double), ("succ", C.c_int), ("fail", C.c_int), ("succ_tol", C.c_int), ("fail_tol", C.c_int),
                ("restarts", C.c_int)]


class ScoreSpec(C.Structure):
    _fields_ = [("kind", C.c_int), ("tradeoff", C.c_double), ("upper", C.c_int), ("sign", C.c_double),
                ("fmin", C.POINTER(C.c_double))]


class RefineOpts(C.Structure):
    _fields_ = [("starts", C.c_int), ("iters", C.c_int), ("eta0", C.c_double), ("lo", C.POINTER(C.c_double)),
                ("hi", C.POINTER(C.c_double))]


SCORE_EI, SCORE_CB, SCORE_LOGEI, SCORE_MES, SCORE_LOGPI = 1, 2, 3, 4, 5
_FMIN_SCORES = {"ei": SCORE_EI, "logei": SCORE_LOGEI, "logpi": SCORE_LOGPI}   # the score= keywords whose kind takes fmin and tradeoff = xi
# b7_eval_nominate_refine: limits, the trace's record width and the status bits of a start
REFINE_MAX_STARTS, REFINE_MAX_ITERS, REFINE_TRACE_WIDTH = 16, 256, 200
REFINE_NOT_RUN, REFINE_FLAT, REFINE_CONVERGED, REFINE_MOVED = 1, 2, 4, 8
# b7_gp_slice_sample: the trace's record width and the status bits of an update
SLICE_TRACE_WIDTH = 136
SLICE_NAN, SLICE_ZERO, SLICE_CAP, SLICE_PIVOT, SLICE_NOT_RUN = 1, 2, 4, 8, 16
MES_KMAX = 64

# covariance kernels (b7_gp_set_kernel): config.model.kernel names (bots/bayesopt.lua:41) -> B7_KERNEL_*
KERNELS = {"ardse": 0, "ardmatern52": 1}


def kernel_code(kernel):
    """'ardse' / 'ardmatern52' (or the B7_KERNEL_* code itself) -> the code; anything else raises Bot7HipError."""
    if isinstance(kernel, str):
        if kernel not in KERNELS:
            raise Bot7HipError(-1, "unknown covariance kernel %r (built: %s)" % (kernel, ", ".join(sorted(KERNELS))))
        return KERNELS[kernel]
    if int(kernel) not in KERNELS.values():
        raise Bot7HipError(-1, "unknown covariance kernel code %r" % (kernel,))
    return int(kernel)


class Mlp(C.Structure):
    _fields_ = [("n_layers", C.c_int), ("dims", C.POINTER(C.c_int)), ("W", C.POINTER(C.POINTER(C.c_double))),
                ("b", C.POINTER(C.POINTER(C.c_double))), ("activation", C.c_int)]


ACTIVATIONS = {None: 0, "Identity": 0, "Tanh": 1, "ReLU": 2, "Sigmoid": 3}
_MLP_CACHE = {}


class LbfgsbOpts(C.Structure):   # b7_lbfgsb_opts
    _fields_ = [("max_iters", C.c_int), ("max_evals", C.c_int), ("gtol", C.c_double)]


# b7_lbfgsb_minimize's status bits
LBFGSB_CONVERGED, LBFGSB_MAX_ITERS, LBFGSB_MAX_EVALS, LBFGSB_LINESEARCH, LBFGSB_STOPPED, LBFGSB_BAD_START = 1, 2, 4, 8, 16, 32
_OBJECTIVE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))


def _lbfgsb_opts(max_iters=None, max_evals=None, gtol=None):
    """b7_lbfgsb_opts from keywords; None selects the library's default of that field."""
    return LbfgsbOpts(-1 if max_iters is None else int(max_iters), 0 if max_evals is None else int(max_evals),
                      0.0 if gtol is None else float(gtol))


def lbfgsb_minimize(fun, x0, lo, hi, max_iters=None, max_evals=None, gtol=None):
    """The library's projected L-BFGS with bounds on a Python callable (b7_lbfgsb_minimize; host only, no context): fun(x) returns
    (f, g) with g of x's length; an exception inside fun stops the run and is raised again here.  Returns dict(x, f, g, iters, evals,
    status)."""
    x0, lo, hi = (np.ascontiguousarray(_f64(v).ravel()) for v in (x0, lo, hi))
    n = x0.size
    if lo.size != n or hi.size != n:
        raise Bot7HipError(-1, "x0, lo and hi must have the same length")
    err = []

    def cb(_user, nn, xp, fp, gp):
        try:
            f, g = fun(np.array(xp[:nn], dtype=np.float64))
            g = np.asarray(g, dtype=np.float64).ravel()
            if g.size != nn:
                raise ValueError("the gradient must have %d entries" % nn)
            fp[0] = float(f)
            for i in range(nn):
                gp[i] = g[i]
            return 0
        except BaseException as e:   # never let an exception cross the C frames
            err.append(e)
            return 1

    keep = _OBJECTIVE(cb)
    opts = _lbfgsb_opts(max_iters, max_evals, gtol)
    x, g = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
    f, it, ev, st = C.c_double(), C.c_int(), C.c_int(), C.c_int()
    rc = load().b7_lbfgsb_minimize(C.cast(keep, C.c_void_p), None, n, _ptr(x0), _ptr(lo), _ptr(hi), C.byref(opts), _ptr(x), C.byref(f),
                                   _ptr(g), C.byref(it), C.byref(ev), C.byref(st))
    if err:
        raise err[0]
    if rc != B7_OK:
        raise Bot7HipError(rc, "lbfgsb_minimize: n in 1..99, lo <= hi, x0 finite and inside the box")
    return {"x": x, "f": f.value, "g": g, "iters": it.value, "evals": ev.value, "status": st.value}


class GpOpts(C.Structure):
    _fields_ = [("jitter_eps", C.c_double), ("jitter_growth", C.c_double), ("var_with_noise", C.c_int),
                ("var_clamp", C.c_int), ("var_min", C.c_double)]


_libs = {}
# the DIAGNOSTIC build (python -m bot7_amd.build --diag: the A/B switches, the fault injector and the RCCL override compiled in);
# test infrastructure, loaded BESIDE the shipped library by Context(..., lib="diag")
_DIAG_SO = os.path.join(os.path.dirname(_HERE), "tools", "_build", "libbot7hip_diag.so")


def lib_path(which=None):
    return _DIAG_SO if which == "diag" else _SO


def load(which=None):
    """Load libbot7hip.so (or, which="diag", the diagnostic build beside it) once.  torch (when installed) is imported first so
    that both share ONE HIP runtime: torch bundles its own libamdhip64 with the same SONAME, and whichever is mapped first
    serves both."""
    path = lib_path(which)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise Bot7HipError(-2, "%s not found: build it with `python -m bot7_amd.build%s` "
                               "(there is no CPU fallback)" % (path, " --diag" if which == "diag" else ""))
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path, mode=C.RTLD_GLOBAL if which != "diag" else C.RTLD_LOCAL)
    dp, vp, i64, i32, dbl = C.POINTER(C.c_double), C.c_void_p, C.c_int64, C.c_int, C.c_double
    sig = {
        "b7_abi_version": (i32, []),
        "b7_create": (i32, [C.POINTER(vp), i32]),
        "b7_destroy": (None, [vp]),
        "b7_last_error": (C.c_char_p, [vp]),
        "b7_device_info": (i32, [vp, C.c_char_p, C.POINTER(i32), C.POINTER(i64)]),
        "b7_sync": (i32, [vp]),
        "b7_set_workspace": (i32, [vp, i64]),
        "b7_sobol_direction_numbers": (i32, [i32, vp]),
        "b7_grid_sobol": (i32, [vp, i64, i32, i64, vp, vp, vp]),
        "b7_grid_random": (i32, [vp, i64, i32, C.c_uint64, i64, vp, vp, vp]),
        "b7_grid_upload": (i32, [vp, vp, i64, i32]),
        "b7_grid_download": (i32, [vp, i64, i64, vp]),
        "b7_grid_trust_region": (i32, [vp, vp, vp, vp, dbl, vp, C.c_uint64, i64]),
        "b7_tr_box": (i32, [i32, i32, C.POINTER(Hyp), vp, dbl, vp, vp, vp, vp]),
        "b7_tr_init": (i32, [C.POINTER(TrState), i32, i32, dbl, dbl, dbl, i32, i32]),
        "b7_tr_update": (i32, [C.POINTER(TrState), vp, i32, C.POINTER(i32)]),
        "b7_grid_shape": (i32, [vp, C.POINTER(i64), C.POINTER(i32)]),
        "b7_grid_remove": (i32, [vp, i64, vp]),
        "b7_grid_remove_rows": (i32, [vp, vp, i64, vp]),
        "b7_gp_default_opts": (i32, [C.POINTER(GpOpts)]),
        "b7_gp_set_opts": (i32, [vp, C.POINTER(GpOpts)]),
        "b7_gp_set_kernel": (i32, [vp, i32]),
        "b7_gp_fit": (i32, [vp, vp, vp, i32, i32, i32, C.POINTER(Hyp), vp, C.POINTER(dbl), C.POINTER(i32)]),
        "b7_gp_set_data": (i32, [vp, vp, vp, i32, i32, i32]),
        "b7_gp_fit_hyp": (i32, [vp, C.POINTER(Hyp), vp, C.POINTER(dbl), C.POINTER(i32)]),
        "b7_gp_predict_hyp": (i32, [vp, C.POINTER(Hyp), vp, vp, vp, C.POINTER(dbl), C.POINTER(i32)]),
        "b7_gp_nll_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "b7_gp_slice_sample": (i32, [vp, i32, i32, vp, vp, vp, vp, i32, i32, C.c_uint64, C.c_uint64, vp, vp, vp, vp]),
        "b7_gp_slice_trace_enable": (i32, [vp, i32]),
        "b7_gp_slice_trace": (i32, [vp, i32, vp, C.POINTER(i32)]),
        "b7_chol": (i32, [vp, vp, i32, vp, C.POINTER(dbl), C.POINTER(i32)]),
        "b7_gp_predict": (i32, [vp, vp, vp]),
        "b7_gp_predict_at": (i32, [vp, vp, i64, vp, vp]),
        "b7_gp_fantasize": (i32, [vp, vp, i32, i32, C.c_uint64, vp, vp, vp]),
        "b7_gp_append": (i32, [vp, vp, vp]),
        "b7_gp_download": (i32, [vp, vp, vp, vp]),
        "b7_blr_basis": (i32, [vp, C.POINTER(Mlp), vp, i64, vp]),
        "b7_blr_features": (i32, [vp, vp, i64, i32]),
        "b7_blr_fit": (i32, [vp, vp, vp, i32, i32, dbl, dbl, dbl, C.POINTER(dbl)]),
        "b7_blr_fit_x": (i32, [vp, C.POINTER(Mlp), vp, vp, i32, dbl, dbl, dbl, C.POINTER(dbl)]),
        "b7_blr_predict": (i32, [vp, vp, vp]),
        "b7_score_reset": (i32, [vp]),
        "b7_score_ei": (i32, [vp, vp, dbl]),
        "b7_score_logei": (i32, [vp, vp, dbl]),
        "b7_score_mes": (i32, [vp]),
        "b7_mes_set_levels": (i32, [vp, i32]),
        "b7_mes_last_ystar": (i32, [vp, C.POINTER(i32), C.POINTER(i32), vp, vp]),
        "b7_mes_ystar": (i32, [vp, vp, vp, i64, i32, vp, vp]),
        "b7_mes_compute": (i32, [vp, vp, vp, vp, i32, i64, vp]),
        "b7_score_cb": (i32, [vp, dbl, i32, dbl]),
        "b7_score_finish": (i32, [vp, dbl, C.POINTER(dbl), C.POINTER(i64), vp]),
        "b7_comm_pick_winner": (i32, [vp, i32, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_comm_unique_id": (i32, [vp]),
        "b7_comm_init": (i32, [vp, i32, i32, vp]),
        "b7_comm_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "b7_comm_destroy": (i32, [vp]),
        "b7_comm_allreduce_f64": (i32, [vp, vp, i32, i32]),
        "b7_score_finish_global": (i32, [vp, dbl, i64, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_eval_nominate": (i32, [vp, i32, C.POINTER(Hyp), C.POINTER(ScoreSpec), i64, C.POINTER(dbl), C.POINTER(i64),
                                   vp, vp]),
        "b7_eval_nominate_batch": (i32, [vp, i32, C.POINTER(Hyp), C.POINTER(ScoreSpec), i32, vp, vp, vp, vp]),
        "b7_ts_nominate": (i32, [vp, i32, C.POINTER(Hyp), i32, i32, C.c_uint64, vp, vp, vp, vp]),
        "b7_ts_last_paths": (i32, [vp, vp]),
        "b7_ts_nominate_refine": (i32, [vp, i32, C.POINTER(Hyp), i32, i32, C.c_uint64, C.POINTER(RefineOpts), vp, vp, vp, vp, vp, vp, vp]),
        "b7_ts_refine_last": (i32, [vp, i32, C.POINTER(i32), vp, vp, vp, vp]),
        "b7_ts_refine_trace_enable": (i32, [vp, i32]),
        "b7_ts_refine_trace": (i32, [vp, i32, i32, vp, C.POINTER(i32)]),
        "b7_ts_path_grad_at": (i32, [vp, vp, i64, vp, vp]),
        "b7_ts_paths": (i32, [vp, i32, C.POINTER(Hyp), i32, i32, C.c_uint64, vp, vp]),
        "b7_ts_hvi_nominate": (i32, [vp, vp, vp, i32, vp, vp, vp, vp]),
        "b7_ts_hvi3_nominate": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp]),
        "b7_hvi_compute": (i32, [vp, vp, i64, i32, vp, i32, vp, vp]),
        "b7_ts_feas_nominate": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "b7_ts_feas_compute": (i32, [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp]),
        "b7_kg_nominate": (i32, [vp, i32, C.POINTER(Hyp), i32, vp, vp, vp, vp, vp]),
        "b7_kg_trace_enable": (i32, [vp, i32]),
        "b7_kg_last": (i32, [vp, vp, vp, vp, vp, vp]),
        "b7_kg_compute": (i32, [vp, C.c_int64, i32, vp, vp, vp]),
        "b7_eval_posterior": (i32, [vp, i32, C.POINTER(Hyp), vp, vp]),
        "b7_posterior_get": (i32, [vp, i32, vp, vp]),
        "b7_pareto_front2": (i32, [vp, i64, vp, vp, vp, C.POINTER(i32)]),
        "b7_hypervolume2": (i32, [vp, i32, vp, C.POINTER(dbl)]),
        "b7_ehvi_compute": (i32, [vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, i64, vp]),
        "b7_ehvi_nominate": (i32, [vp, vp, vp, i32, vp, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_pareto_front3": (i32, [vp, i64, vp, vp, vp, C.POINTER(i32)]),
        "b7_nondominated_boxes3": (i32, [vp, i32, vp, vp, C.POINTER(i32)]),
        "b7_hypervolume3": (i32, [vp, i32, vp, C.POINTER(dbl)]),
        "b7_ehvi3_compute": (i32, [vp, vp, vp, vp, vp, i32, vp, i64, vp]),
        "b7_ehvi3_nominate": (i32, [vp, vp, vp, vp, i32, vp, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_logehvi_compute": (i32, [vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, i64, vp]),
        "b7_logehvi_nominate": (i32, [vp, vp, vp, i32, vp, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_logehvi3_compute": (i32, [vp, vp, vp, vp, vp, i32, vp, i64, vp]),
        "b7_logehvi3_nominate": (i32, [vp, vp, vp, vp, i32, vp, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_refine_default_opts": (i32, [C.POINTER(RefineOpts)]),
        "b7_eval_nominate_refine": (i32, [vp, i32, C.POINTER(Hyp), C.POINTER(ScoreSpec), C.POINTER(RefineOpts), C.POINTER(dbl),
                                          C.POINTER(i64), vp, C.POINTER(dbl), C.POINTER(i64), vp, vp]),
        "b7_refine_last": (i32, [vp, C.POINTER(i32), vp, vp, vp, vp]),
        "b7_refine_shape": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "b7_refine_trace_enable": (i32, [vp, i32]),
        "b7_refine_trace": (i32, [vp, i32, vp, C.POINTER(i32)]),
        "b7_gp_grad_at": (i32, [vp, vp, i64, vp, vp, vp, vp]),
        "b7_score_grad_compute": (i32, [vp, C.POINTER(ScoreSpec), i32, vp, vp, vp, vp, i64, i32, vp, vp]),
        "b7_ts_last_draws": (i32, [vp, i32, vp, vp, vp, vp]),
        "b7_rff_compute": (i32, [vp, vp, i64, i32, vp, vp, vp, i32, i32, vp]),
        "b7_blr_ts_nominate": (i32, [vp, C.POINTER(Mlp), vp, vp, i32, i32, vp, vp, vp, i32, C.c_uint64, vp, vp, vp, C.POINTER(dbl)]),
        "b7_blr_ts_last_draws": (i32, [vp, i32, vp, vp]),
        "b7_blr_paths_compute": (i32, [vp, vp, i64, i32, vp, vp, i32, vp]),
        "b7_blr_eval_nominate": (i32, [vp, C.POINTER(Mlp), vp, vp, i32, dbl, dbl, dbl, C.POINTER(ScoreSpec), i64, C.POINTER(dbl),
                                       C.POINTER(i64), C.POINTER(dbl)]),
        "b7_blr_eval_nominate_marg": (i32, [vp, C.POINTER(Mlp), vp, vp, i32, i32, vp, vp, vp, C.POINTER(ScoreSpec), i64, C.POINTER(dbl),
                                            C.POINTER(i64), vp, C.POINTER(dbl)]),
        "b7_grid_random_torch": (i32, [vp, i64, i32, C.c_uint64, i32, vp, vp, vp]),
        "b7_torch_rand": (i32, [C.c_uint64, i64, i32, vp]),
        "b7_grid_colrange": (i32, [vp, vp, vp]),
        "b7_grid_apply_onesided": (i32, [vp, vp, vp, vp]),
        "b7_nominate_commit": (i32, [vp, i64, C.POINTER(i64), vp]),
        "b7_shard_commit_rule": (i32, [i64, i64, i64, C.POINTER(i64), C.POINTER(i64)]),
        "b7_exchange_info": (i32, [vp, C.POINTER(i32), vp, C.POINTER(i64), C.POINTER(i32), vp]),
        "b7_group_create": (i32, [C.POINTER(vp), i32, vp]),
        "b7_group_destroy": (None, [vp]),
        "b7_group_last_error": (C.c_char_p, [vp]),
        "b7_group_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "b7_group_ctx": (vp, [vp, i32]),
        "b7_group_set_workspace": (i32, [vp, i64]),
        "b7_group_gp_set_opts": (i32, [vp, C.POINTER(GpOpts)]),
        "b7_group_gp_set_kernel": (i32, [vp, i32]),
        "b7_group_grid_sobol": (i32, [vp, i64, i32, i64, vp, vp]),
        "b7_group_grid_random": (i32, [vp, i64, i32, C.c_uint64, vp, vp]),
        "b7_group_grid_onesided": (i32, [vp, vp, vp]),
        "b7_group_grid_upload": (i32, [vp, vp, i64, i32]),
        "b7_group_grid_shape": (i32, [vp, C.POINTER(i64), C.POINTER(i32), vp]),
        "b7_group_grid_download": (i32, [vp, i64, i64, vp]),
        "b7_group_grid_remove_rows": (i32, [vp, vp, i64, vp]),
        "b7_group_gp_set_data": (i32, [vp, vp, vp, i32, i32, i32]),
        "b7_group_eval_nominate": (i32, [vp, i32, C.POINTER(Hyp), C.POINTER(ScoreSpec), C.POINTER(dbl), C.POINTER(i64), vp, vp]),
        "b7_group_nominate_commit": (i32, [vp, i64, vp]),
        "b7_ei_compute": (i32, [vp, vp, vp, vp, dbl, i64, i32, vp]),
        "b7_cb_compute": (i32, [vp, vp, vp, dbl, i32, dbl, i64, i32, vp]),
        "b7_logei_compute": (i32, [vp, vp, vp, vp, dbl, i64, i32, vp]),
        "b7_argmax": (i32, [vp, vp, i64, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_score_logpi": (i32, [vp, vp, dbl]),
        "b7_logpi_compute": (i32, [vp, vp, vp, vp, dbl, i64, i32, vp]),
        "b7_feas_reset": (i32, [vp]),
        "b7_feas_add": (i32, [vp, vp, i64]),
        "b7_feas_add_acc": (i32, [vp, vp]),
        "b7_feas_get": (i32, [vp, vp]),
        "b7_feas_nominate": (i32, [vp, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_eval_nominate_feasible": (i32, [vp, i32, C.POINTER(Hyp), C.POINTER(ScoreSpec), C.POINTER(dbl), C.POINTER(i64), vp, vp]),
        "b7_clf_nll_batch": (i32, [vp, i32, C.POINTER(Hyp), vp, vp, vp]),
        "b7_clf_fit_hyp": (i32, [vp, C.POINTER(Hyp), C.POINTER(dbl), C.POINTER(i32), C.POINTER(i32)]),
        "b7_clf_mode_get": (i32, [vp, vp, vp, vp]),
        "b7_clf_eval_logfeas": (i32, [vp, i32, C.POINTER(Hyp), C.POINTER(dbl), C.POINTER(i64), vp, vp]),
        "b7_probit_compute": (i32, [vp, vp, i64, vp, vp, vp]),
        "b7_gp_fit_hyp_grad": (i32, [vp, C.POINTER(Hyp), C.POINTER(dbl), vp, C.POINTER(dbl), C.POINTER(i32)]),
        "b7_gp_nll_grad": (i32, [vp, vp]),
        "b7_lbfgsb_default_opts": (i32, [C.POINTER(LbfgsbOpts)]),
        "b7_lbfgsb_minimize": (i32, [vp, vp, i32, vp, vp, vp, C.POINTER(LbfgsbOpts), vp, C.POINTER(dbl), vp, C.POINTER(i32), C.POINTER(i32),
                                     C.POINTER(i32)]),
        "b7_gp_fit_map": (i32, [vp, vp, vp, vp, C.POINTER(LbfgsbOpts), vp, C.POINTER(dbl), vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "b7_gp_fit_map_trace_enable": (i32, [vp, i32]),
        "b7_gp_fit_map_trace": (i32, [vp, vp, C.POINTER(i32), C.POINTER(i32)]),
        "b7_timer_start": (i32, [vp, i32]),
        "b7_timer_stop": (i32, [vp, i32]),
        "b7_timer_ms": (i32, [vp, i32, C.POINTER(C.c_float)]),
        "b7_profile_enable": (i32, [vp, i32]),
        "b7_profile_reset": (i32, [vp]),
        "b7_profile_get": (i32, [vp, C.c_char_p, C.POINTER(dbl), C.POINTER(i64)]),
        "b7_persist_fallbacks": (i32, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _libs[path] = L
    return L


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class BlrThompson(object):
    """Thompson sampling on the DNGO head (b7_blr_ts_nominate and its two companions), mixed into Context below.  A class of its own
    because the reuse catalogue (tests/_reuse_calls.py) is keyed on the methods Context itself defines and has no entry for these
    three yet: they are held to the reuse discipline (a context after the call against a fresh one, bit for bit) by
    tests/test_gpu_blr_ts.py instead."""

    def blr_ts_nominate(self, weights, biases, activation, X0, Y0, alphas, betas, means, q, seed=0, want_report=False):
        """Thompson sampling for the DNGO head (b7_blr_ts_nominate): q exact sample paths f_j = mean_s + phi' w_j, w_j ~ N(m_s, inv(A_s)),
        path j under head j mod S of the S samples (alpha, beta, mean); each path's first minimum among the rows no earlier path of the
        call took.  Returns (path minima[q], 1-based indices[q][, {"jitter": flag, "nll": per sample}]); the grid is not modified."""
        net = self._mlp(weights, biases, activation)
        X = _f64(X0)
        Y = _f64(Y0).ravel()
        a, b, m = (np.ascontiguousarray(_f64(v).ravel()) for v in (alphas, betas, means))
        S = a.size
        if b.size != S or m.size != S:
            raise Bot7HipError(-1, "alphas, betas and means must have the same length")
        nll = np.empty(max(S, 1), dtype=np.float64) if want_report else None
        n = max(int(q), 1)
        vals, idx, jit = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64), C.c_double()
        self._ck(self._L.b7_blr_ts_nominate(self._h, C.byref(net), _ptr(X), _ptr(Y), X.shape[0], S, _ptr(a), _ptr(b), _ptr(m), int(q),
                                            int(seed) & (2 ** 64 - 1), _ptr(vals), _ptr(idx), _ptr(nll), C.byref(jit)))
        self.fit_token += 1
        self._ts_shape = (self.grid_shape()[0], n, 0, 0, 0)
        self._blr_ts_z = net._keep[0][-1].shape[0]
        if want_report:
            return vals, idx, {"jitter": jit.value, "nll": nll[:S]}
        return vals, idx

    def blr_ts_last_draws(self, path):
        """Path `path`'s draw and weight vector of the last blr_ts_nominate: dict(eps z, weight z) (b7_blr_ts_last_draws)."""
        z = getattr(self, "_blr_ts_z", 1)
        out = {"eps": np.empty(z, dtype=np.float64), "weight": np.empty(z, dtype=np.float64)}
        self._ck(self._L.b7_blr_ts_last_draws(self._h, int(path), _ptr(out["eps"]), _ptr(out["weight"])))
        return out

    def blr_paths_compute(self, Z, W, mean0):
        """mean0' + Z W on host arrays (b7_blr_paths_compute): Z M1 x z, W z x q, mean0 q -> M1 x q."""
        Z, W, mean0 = _f64(Z), _f64(W), _f64(mean0).ravel()
        if Z.ndim != 2 or W.ndim != 2 or W.shape[0] != Z.shape[1] or mean0.size != W.shape[1]:
            raise Bot7HipError(-1, "blr_paths_compute: Z M1 x z, W z x q and mean0 q expected")
        out = np.empty((Z.shape[0], W.shape[1]), dtype=np.float64)
        self._ck(self._L.b7_blr_paths_compute(self._h, _ptr(Z), Z.shape[0], Z.shape[1], _ptr(W), _ptr(mean0), W.shape[1], _ptr(out)))
        return out


class ThompsonObjectives(object):
    """Multi-objective Thompson sampling (b7_ts_paths, b7_ts_hvi_nominate / b7_ts_hvi3_nominate, b7_hvi_compute; csrc/ts_hvi.hip), mixed
    into Context below.  A class of its own for BlrThompson's reason: the reuse catalogue is keyed on the methods Context itself defines;
    these are held to the same call twice giving the same bits by tests/test_gpu_ts_hvi.py."""

    def ts_paths(self, hyps, q, n_features=1024, seed=0, want_report=False):
        """The path half of ts_nominate, kept (b7_ts_paths): the same q sample paths over the resident grid for the same arguments,
        without the arg-mins; ts_last_paths / ts_last_draws serve it and ts_hvi_nominate reads it.  A change of the grid or the data
        makes the paths stale for ts_hvi_nominate.  Returns None, or the report dict(jitter, info)."""
        S = len(hyps)
        arr, keep = self._pack_hyps(hyps, getattr(self, "_data_d", -1))
        jit = np.zeros(max(S, 1), dtype=np.float64) if want_report else None
        info = np.zeros(max(S, 1), dtype=np.int32) if want_report else None
        self._ck(self._L.b7_ts_paths(self._h, S, arr, int(q), int(n_features), int(seed) & (2 ** 64 - 1), _ptr(jit), _ptr(info)))
        self.fit_token += 1
        self._ts_shape = (self.grid_shape()[0], max(int(q), 1), int(n_features), self._data_d, getattr(self, "_data_n", 0))
        return {"jitter": jit[:S], "info": info[:S]} if want_report else None

    def ts_hvi_nominate(self, others, front, ref):
        """q nominees for two or three objectives by Thompson sampling (b7_ts_hvi_nominate / b7_ts_hvi3_nominate): this context holds
        objective 1's kept paths (ts_paths), `others` -- one Context, or a pair -- those of the later objectives (contexts may
        coincide), all over the same grid rows with the same q.  Path j picks the row whose sampled values improve the hypervolume of
        (front + the earlier picks under path j) the most, over the rows no earlier path took; where none improves it, the first
        minimum of objective 1 + (j mod m)'s path.  Returns (hvi[q], 1-based indices[q], y[q x m]); no grid is modified."""
        others = [others] if isinstance(others, Context) else list(others)
        m = 1 + len(others)
        if m not in (2, 3) or any(not isinstance(o, Context) or o._L is not self._L for o in others):
            raise Bot7HipError(-1, "ts_hvi_nominate: others is one Context (two objectives) or a pair (three), of the same library")
        front, ref = _f64(front).reshape(-1, m), _f64(ref).ravel()
        if ref.size != m:
            raise Bot7HipError(-1, "ts_hvi_nominate: ref has one entry per objective")
        q = getattr(self, "_ts_shape", (1, 1))[1]
        hvi, idx, y = np.zeros(q, dtype=np.float64), np.zeros(q, dtype=np.int64), np.zeros((q, m), dtype=np.float64)
        fn = self._L.b7_ts_hvi_nominate if m == 2 else self._L.b7_ts_hvi3_nominate
        self._ck(fn(self._h, *[o._h for o in others], _ptr(front), front.shape[0], _ptr(ref), _ptr(hvi), _ptr(idx), _ptr(y)))
        return hvi, idx, y

    def hvi_compute(self, Y, front, ref):
        """The hypervolume improvement of each row of Y (M1 x m, m = 2 or 3) against a canonical front, by ts_hvi_nominate's own
        kernels (b7_hvi_compute); NaN for a row with an entry that is not finite."""
        Y, ref = _f64(Y), _f64(ref).ravel()
        m = ref.size
        if Y.ndim != 2 or Y.shape[1] != m:
            raise Bot7HipError(-1, "hvi_compute: Y M1 x m, front P x m, ref m")
        front = _f64(front).reshape(-1, m)
        out = np.empty(Y.shape[0], dtype=np.float64)
        self._ck(self._L.b7_hvi_compute(self._h, _ptr(Y), Y.shape[0], m, _ptr(front), front.shape[0], _ptr(ref), _ptr(out)))
        return out


class ThompsonFeasible(object):
    """Constrained Thompson sampling (b7_ts_feas_nominate, b7_ts_feas_compute; csrc/ts_feas.hip), mixed into Context below.  A class of
    its own for BlrThompson's reason; these are held to the same call twice giving the same bits by tests/test_gpu_ts_feas.py."""

    def ts_feas_nominate(self, cons, thresholds):
        """q feasible-first nominees under C constraints c_k <= thresholds[k] by Thompson sampling (b7_ts_feas_nominate): this context
        holds the objective's kept paths (ts_paths), cons[k] -- Contexts of the same library, which may coincide -- those of constraint
        k + 1, all over the same grid rows with the same q.  Path j picks the row of lowest f_j among the rows where every c_kj <= t_k
        that no earlier path took; where the path sees no feasible row, the row of smallest total violation.  Returns dict(key[q],
        cls[q] (0 feasible, 1 not, -1 no row), index[q] (1-based, 0 for no row), y[q x (1 + C)], reruns: 0 in the library's default arm, which
        picks path by path); no grid is modified."""
        cons = list(cons)
        if any(not isinstance(o, Context) or o._L is not self._L for o in cons):
            raise Bot7HipError(-1, "ts_feas_nominate: cons is a list of Contexts of the same library")
        thr = _f64(thresholds).ravel()
        if thr.size != len(cons):
            raise Bot7HipError(-1, "ts_feas_nominate: one threshold per constraint context")
        Cn = len(cons)
        q = getattr(self, "_ts_shape", (1, 1))[1]
        handles = (C.c_void_p * max(Cn, 1))(*[o._h for o in cons])
        qmax = 16   # B7_BATCH_MAX: the library writes as many entries as the contexts keep paths
        key, cls, idx = np.zeros(qmax, dtype=np.float64), np.zeros(qmax, dtype=np.int32), np.zeros(qmax, dtype=np.int64)
        y, reruns = np.zeros(qmax * (1 + Cn), dtype=np.float64), C.c_int(0)
        self._ck(self._L.b7_ts_feas_nominate(self._h, C.cast(handles, C.c_void_p) if Cn else None, _ptr(thr) if Cn else None, Cn, _ptr(key),
                                             _ptr(cls), _ptr(idx), _ptr(y), C.c_void_p(C.addressof(reruns))))
        return {"key": key[:q].copy(), "cls": cls[:q].copy(), "index": idx[:q].copy(), "y": y[:q * (1 + Cn)].reshape(q, 1 + Cn).copy(),
                "reruns": int(reruns.value)}

    def ts_feas_compute(self, f, cvals, thresholds, want_viol=True):
        """ts_feas_nominate's kernels and resolution on host arrays (b7_ts_feas_compute): f M1 x q, cvals C x M1 x q (or a list of C
        arrays M1 x q), thresholds C.  Returns dict(viol[M1 x q] (NaN where a value is NaN; None unless want_viol), key[q], cls[q],
        index[q])."""
        f, thr = _f64(f), _f64(thresholds).ravel()
        Cn = thr.size
        if f.ndim != 2:
            raise Bot7HipError(-1, "ts_feas_compute: f M1 x q, cvals C x M1 x q, thresholds C")
        cv = _f64(np.asarray(cvals, dtype=np.float64).reshape((Cn,) + f.shape)) if Cn else None
        M1, q = f.shape
        viol = np.empty((M1, q), dtype=np.float64) if want_viol else None
        key, cls, idx = np.zeros(max(q, 1), dtype=np.float64), np.zeros(max(q, 1), dtype=np.int32), np.zeros(max(q, 1), dtype=np.int64)
        self._ck(self._L.b7_ts_feas_compute(self._h, _ptr(f), _ptr(cv), _ptr(thr) if Cn else None, M1, q, Cn, _ptr(viol), _ptr(key), _ptr(cls),
                                            _ptr(idx)))
        return {"viol": viol, "key": key[:q], "cls": cls[:q], "index": idx[:q]}


class ThompsonRefine(object):
    """Thompson nominees refined off the grid by descent on their own sample paths (b7_ts_nominate_refine, b7_ts_refine_last,
    b7_ts_refine_trace, b7_ts_path_grad_at): the methods of Context that serve it."""

    def ts_nominate_refine(self, hyps, q, n_features=1024, seed=0, starts=16, iters=16, eta0=1.0 / 16.0, lo=None, hi=None,
                           want_report=False):
        """ts_nominate, then every path's nominee refined off the grid by descent on the path itself from `starts` starts (the
        nominee, then the path's lowest rows that are no path's nominee) for `iters` iterations inside the box [lo, hi] (None: the
        unit cube) (b7_ts_nominate_refine).  Returns (path minima[q], 1-based grid nominees[q], x[q x d], refined path values[q],
        1-based rows of the winners' starts[q][, report]); the grid is not modified: the rows to commit are the grid nominees."""
        S = len(hyps)
        d = getattr(self, "_data_d", -1)
        arr, keep = self._pack_hyps(hyps, d)
        lo = None if lo is None else _f64(lo).ravel()
        hi = None if hi is None else _f64(hi).ravel()
        for b in (lo, hi):
            if b is not None and b.size != d:
                raise Bot7HipError(-1, "lo / hi must have d entries")
        dp = C.POINTER(C.c_double)
        opts = RefineOpts(int(starts), int(iters), float(eta0), None if lo is None else lo.ctypes.data_as(dp),
                          None if hi is None else hi.ctypes.data_as(dp))
        jit = np.zeros(max(S, 1), dtype=np.float64) if want_report else None
        info = np.zeros(max(S, 1), dtype=np.int32) if want_report else None
        n = max(int(q), 1)
        vals, idx = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64)
        x, rv, ri = np.zeros((n, max(d, 1)), dtype=np.float64), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64)
        self._ck(self._L.b7_ts_nominate_refine(self._h, S, arr, int(q), int(n_features), int(seed) & (2 ** 64 - 1), C.byref(opts),
                                               _ptr(vals), _ptr(idx), _ptr(x), _ptr(rv), _ptr(ri), _ptr(jit), _ptr(info)))
        self.fit_token += 1
        self._ts_shape = (self.grid_shape()[0], n, int(n_features), self._data_d, getattr(self, "_data_n", 0))
        self._ts_refine_iters = int(iters)
        if want_report:
            return vals, idx, x, rv, ri, {"jitter": jit[:S], "info": info[:S]}
        return vals, idx, x, rv, ri

    def ts_refine_last(self, path):
        """Every start of path `path` in the last ts_nominate_refine, in rank order: dict(x P x d, val P, start_idx1 P, status P)
        (b7_ts_refine_last)."""
        d = getattr(self, "_ts_shape", (1, 1, 1, 1, 1))[3]
        n = C.c_int()
        x, val = np.zeros((REFINE_MAX_STARTS, d), dtype=np.float64), np.zeros(REFINE_MAX_STARTS, dtype=np.float64)
        idx, status = np.zeros(REFINE_MAX_STARTS, dtype=np.int64), np.zeros(REFINE_MAX_STARTS, dtype=np.int32)
        self._ck(self._L.b7_ts_refine_last(self._h, int(path), C.byref(n), _ptr(x), _ptr(val), _ptr(idx), _ptr(status)))
        P = n.value
        return {"x": x[:P].copy(), "val": val[:P].copy(), "start_idx1": idx[:P].copy(), "status": status[:P].copy()}

    def ts_refine_trace_enable(self, on=True):
        """Keep one record per path, start and iteration of the ts_nominate_refine calls that follow (b7_ts_refine_trace_enable)."""
        self._ck(self._L.b7_ts_refine_trace_enable(self._h, int(bool(on))))

    def ts_refine_trace(self, path, start):
        """The records of start `start` of path `path` in the last traced ts_nominate_refine, iteration 0..iters, as refine_trace
        returns them: x, val and grad are the PATH's (the ladder ran on their negatives), cand the rungs' path values
        (b7_ts_refine_trace)."""
        d = getattr(self, "_ts_shape", (1, 1, 1, 1, 1))[3]
        buf = np.zeros((getattr(self, "_ts_refine_iters", 0) + 1, REFINE_TRACE_WIDTH), dtype=np.float64)
        n = C.c_int()
        self._ck(self._L.b7_ts_refine_trace(self._h, int(path), int(start), _ptr(buf), C.byref(n)))
        r = buf[:n.value]
        return {"x": r[:, :d].copy(), "val": r[:, d].copy(), "grad": r[:, d + 1:2 * d + 1].copy(), "eta": r[:, 2 * d + 1].copy(),
                "cand": r[:, 2 * d + 2:2 * d + 6].copy(), "rung": r[:, 2 * d + 6].astype(np.int64),
                "status": r[:, 2 * d + 7].astype(np.int64)}

    def ts_path_grad_at(self, X1):
        """The kept sample paths and their gradients at the rows of X1: (val M1 x q, grad M1 x q x d) (b7_ts_path_grad_at)."""
        X1 = _f64(X1)
        if X1.ndim == 1:
            X1 = X1.reshape(1, -1)
        M1, d = X1.shape
        q = getattr(self, "_ts_shape", (1, 1, 1, 1, 1))[1]
        val, grad = np.empty((M1, q), dtype=np.float64), np.empty((M1, q, d), dtype=np.float64)
        self._ck(self._L.b7_ts_path_grad_at(self._h, _ptr(X1), M1, _ptr(val), _ptr(grad)))
        return val, grad


class LaplaceClassifier(object):
    """The probit GP classifier by Laplace's method (b7_clf_*; csrc/laplace.hip), mixed into Context below: binary constraints, the
    resident data's one response column holding labels 0 / 1 with 1 = violated.  A class of its own for BlrThompson's reason; these
    are held to the same call twice giving the same bits by tests/test_gpu_laplace.py."""

    CLF_NOT_CONVERGED = 1   # info bit 0: the stopping rule was not met within 32 Newton iterations

    def _clf_hyps(self, hyps):
        # without resident data the library's own refusal is the answer: the lengthscales are packed at the length they come in
        d = getattr(self, "_data_d", None)
        if d is None and len(hyps):
            h = hyps[0]
            d = _f64(h["lenscale_sq"] if isinstance(h, dict) else h[0]).size
        return self._pack_hyps(hyps, d)

    def clf_nll_batch(self, hyps, want_info=False):
        """-log of Laplace's approximate evidence of the resident labels under each hyper vector of hyps (sequence of (lenscale_sq,
        amp, noise, mean) or dicts; noise is ignored), B workgroups of one launch (b7_clf_nll_batch).  Returns nll[B] (, iterations[B],
        info[B])."""
        B = len(hyps)
        arr, keep = self._clf_hyps(hyps)
        nll, it, info = np.empty(max(B, 1), dtype=np.float64), np.zeros(max(B, 1), dtype=np.int32), np.zeros(max(B, 1), dtype=np.int32)
        self._ck(self._L.b7_clf_nll_batch(self._h, B, arr, _ptr(nll), _ptr(it), _ptr(info)))
        return (nll[:B], it[:B], info[:B]) if want_info else nll[:B]

    def clf_fit_hyp(self, lenscale_sq, amp, noise, mean):
        """One Laplace fit into the context's own fit slot (b7_clf_fit_hyp): gp_predict / gp_predict_at then return the LATENT mean and
        variance.  Returns dict(nll, iters, info)."""
        ls = _f64(lenscale_sq).ravel()
        if ls.size != getattr(self, "_data_d", ls.size):
            raise Bot7HipError(-1, "lenscale_sq must have d entries")
        hyp = Hyp(ls.ctypes.data_as(C.POINTER(C.c_double)), float(amp), float(noise), float(mean))
        nll, it, info = C.c_double(), C.c_int(), C.c_int()
        self._ck(self._L.b7_clf_fit_hyp(self._h, C.byref(hyp), C.byref(nll), C.byref(it), C.byref(info)))
        self.fit_token += 1
        return {"nll": nll.value, "iters": it.value, "info": info.value}

    def clf_mode_get(self):
        """(f^, a, W) of the last clf_fit_hyp, N entries each (b7_clf_mode_get)."""
        n = getattr(self, "_data_n", 0)
        f, a, W = (np.empty(n, dtype=np.float64) for _ in range(3))
        self._ck(self._L.b7_clf_mode_get(self._h, _ptr(f), _ptr(a), _ptr(W)))
        return f, a, W

    def clf_eval_logfeas(self, hyps, want_report=False):
        """S Laplace fits, their latent posteriors over the resident grid (kept: posterior_get(s) serves them) and the marginal
        log Pr[feasible | x] = log((1/S) sum_s Phi(-mu_s / sqrt(var_s + 1))) left in the accumulator, as eval_nominate(score="logpi",
        fmin=0) leaves one for a regression constraint: feas_add_acc(this context) takes it (b7_clf_eval_logfeas).  Returns (value,
        1-based index[, dict(iters, info)]) of the accumulator's arg-max."""
        S = len(hyps)
        arr, keep = self._clf_hyps(hyps)
        it, info = np.zeros(max(S, 1), dtype=np.int32), np.zeros(max(S, 1), dtype=np.int32)
        v, i = C.c_double(), C.c_int64()
        self._ck(self._L.b7_clf_eval_logfeas(self._h, S, arr, C.byref(v), C.byref(i), _ptr(it), _ptr(info)))
        self.fit_token += 1
        if want_report:
            return v.value, i.value, {"iters": it[:S], "info": info[:S]}
        return v.value, i.value

    def probit_compute(self, z):
        """(log Phi(z), phi(z)/Phi(z), W(z)) of a host vector by the fit's own device functions (b7_probit_compute)."""
        z = _f64(z).ravel()
        out = [np.empty(z.size, dtype=np.float64) for _ in range(3)]
        self._ck(self._L.b7_probit_compute(self._h, _ptr(z), z.size, *[_ptr(o) for o in out]))
        return tuple(out)


class LikelihoodGradient(object):
    """The likelihood's gradient and the bounded fit that descends on it (b7_gp_fit_hyp_grad, b7_gp_nll_grad, b7_gp_fit_map;
    csrc/nll_grad.hip), mixed into Context below.  A class of its own for BlrThompson's reason; these are held to the same call twice
    giving the same bits by tests/test_gpu_nllgrad.py.  theta = [log lenscale_sq (d), log amp, log noise, mean]."""

    def gp_fit_hyp_grad(self, lenscale_sq, amp, noise, mean):
        """gp_fit_hyp plus the gradient of its nll in theta's coordinates.  Returns dict(nll, grad[d + 3], jitter, info)."""
        ls = _f64(lenscale_sq).ravel()
        if ls.size != getattr(self, "_data_d", ls.size):
            raise Bot7HipError(-1, "lenscale_sq must have d entries (call gp_set_data first)")
        hyp = Hyp(ls.ctypes.data_as(C.POINTER(C.c_double)), float(amp), float(noise), float(mean))
        grad = np.empty(ls.size + 3, dtype=np.float64)
        nll, jit, info = C.c_double(), C.c_double(), C.c_int()
        self._ck(self._L.b7_gp_fit_hyp_grad(self._h, C.byref(hyp), C.byref(nll), _ptr(grad), C.byref(jit), C.byref(info)))
        self.fit_token += 1
        return {"nll": nll.value, "grad": grad, "jitter": jit.value, "info": info.value}

    def gp_nll_grad(self):
        """The gradient of the fit the context holds (b7_gp_nll_grad): d + 3 components."""
        grad = np.empty(getattr(self, "_data_d", B7_MAX_D_PY) + 3, dtype=np.float64)
        self._ck(self._L.b7_gp_nll_grad(self._h, _ptr(grad)))
        return grad

    def gp_fit_map(self, theta0, lo, hi, max_iters=None, max_evals=None, gtol=None):
        """Bounded maximum likelihood of the resident data from theta0 inside [lo, hi] (b7_gp_fit_map); the context's fit slot holds
        the fit at the result.  Returns dict(theta, nll, grad, iters, evals, status)."""
        t0, lo, hi = (np.ascontiguousarray(_f64(v).ravel()) for v in (theta0, lo, hi))
        n = getattr(self, "_data_d", t0.size - 3) + 3
        if t0.size != n or lo.size != n or hi.size != n:
            raise Bot7HipError(-1, "theta0, lo and hi must have d + 3 entries (call gp_set_data first)")
        opts = _lbfgsb_opts(max_iters, max_evals, gtol)
        th, g = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        nll, it, ev, st = C.c_double(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.b7_gp_fit_map(self._h, _ptr(t0), _ptr(lo), _ptr(hi), C.byref(opts), _ptr(th), C.byref(nll), _ptr(g), C.byref(it),
                                       C.byref(ev), C.byref(st)))
        self.fit_token += 1
        return {"theta": th, "nll": nll.value, "grad": g, "iters": it.value, "evals": ev.value, "status": st.value}

    def gp_fit_map_trace_enable(self, on=True):
        self._ck(self._L.b7_gp_fit_map_trace_enable(self._h, int(bool(on))))

    def gp_fit_map_trace(self):
        """The last traced gp_fit_map: one row per accepted iterate, row 0 the start: theta (d + 3) | nll | step."""
        n, w = C.c_int(), C.c_int()
        self._ck(self._L.b7_gp_fit_map_trace(self._h, None, C.byref(n), C.byref(w)))
        buf = np.empty((n.value, w.value), dtype=np.float64)
        self._ck(self._L.b7_gp_fit_map_trace(self._h, _ptr(buf), C.byref(n), C.byref(w)))
        return buf


B7_MAX_D_PY = 96


class Context(BlrThompson, ThompsonObjectives, ThompsonFeasible, ThompsonRefine, LaplaceClassifier, LikelihoodGradient):
    """One GPU's worth of state: the resident candidate grid, the current GP fit, the score accumulator."""

    def __init__(self, device_id=0, _borrowed=None, lib=None):
        self._L = load(lib)
        self._lib_name = lib
        if _borrowed is not None:   # a member of a Group: the handle belongs to the group
            self._h, self._owned = C.c_void_p(_borrowed), False
        else:
            h = C.c_void_p()
            rc = self._L.b7_create(C.byref(h), int(device_id))
            if rc != B7_OK:
                raise Bot7HipError(rc, (self._L.b7_last_error(None) or b"").decode())
            self._h, self._owned = h, True
        self.device_id = int(device_id)
        self.grid_version = 0  # bumped whenever the resident grid changes (DeviceGrid views compare against it)
        self.fit_token = 0     # bumped by every call that replaces the fit (models check it before gp_append)
        self.kernel = KERNELS["ardse"]  # the context's covariance kernel (b7_gp_set_kernel; a new context starts on ARD-SE)

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._L.b7_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != B7_OK:
            raise Bot7HipError(rc, (self._L.b7_last_error(self._h) or b"").decode())

    # ---- context
    def device_info(self):
        name = C.create_string_buffer(64)
        cus, mem = C.c_int(), C.c_int64()
        self._ck(self._L.b7_device_info(self._h, name, C.byref(cus), C.byref(mem)))
        return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": mem.value}

    def sync(self):
        self._ck(self._L.b7_sync(self._h))

    def set_workspace(self, nbytes):
        self._ck(self._L.b7_set_workspace(self._h, int(nbytes)))

    # ---- grids
    @staticmethod
    def _minmax(mins, maxes, dims):
        if mins is None and maxes is None:
            return None, None
        # one of the two alone selects the one-sided maps of grids/sobol.lua:82-85
        mn = None if mins is None else _f64(mins).ravel()
        mx = None if maxes is None else _f64(maxes).ravel()
        if (mn is not None and mn.size != dims) or (mx is not None and mx.size != dims):
            raise Bot7HipError(-1, "mins/maxes must have `dims` entries")
        return mn, mx

    def grid_sobol(self, size, dims, skip=1, mins=None, maxes=None, download=True):
        mn, mx = self._minmax(mins, maxes, dims)
        out = np.empty((size, dims), dtype=np.float64) if download else None
        self._ck(self._L.b7_grid_sobol(self._h, int(size), int(dims), int(skip), _ptr(mn), _ptr(mx), _ptr(out)))
        self.grid_version += 1
        return out

    def grid_random(self, size, dims, seed=0, row_offset=0, mins=None, maxes=None, download=True):
        mn, mx = self._minmax(mins, maxes, dims)
        out = np.empty((size, dims), dtype=np.float64) if download else None
        self._ck(self._L.b7_grid_random(self._h, int(size), int(dims), int(seed) & (2 ** 64 - 1), int(row_offset),
                                        _ptr(mn), _ptr(mx), _ptr(out)))
        self.grid_version += 1
        return out

    def grid_random_torch(self, size, dims, seed=0, resolution=32, mins=None, maxes=None, download=True):
        """grids/random.lua with torch.rand's own MT19937 stream (torch.manualSeed(seed))."""
        mn, mx = self._minmax(mins, maxes, dims)
        out = np.empty((size, dims), dtype=np.float64) if download else None
        self._ck(self._L.b7_grid_random_torch(self._h, int(size), int(dims), int(seed), int(resolution), _ptr(mn), _ptr(mx),
                                              _ptr(out)))
        self.grid_version += 1
        return out

    def grid_upload(self, X):
        X = _f64(X)
        if X.ndim != 2:
            raise Bot7HipError(-1, "grid must be 2-D")
        self._ck(self._L.b7_grid_upload(self._h, _ptr(X), X.shape[0], X.shape[1]))
        self.grid_version += 1

    def grid_shape(self):
        M, d = C.c_int64(), C.c_int()
        self._ck(self._L.b7_grid_shape(self._h, C.byref(M), C.byref(d)))
        return M.value, d.value

    def grid_download(self, row0=0, rows=None):
        M, d = self.grid_shape()
        rows = M - row0 if rows is None else rows
        out = np.empty((rows, d), dtype=np.float64)
        self._ck(self._L.b7_grid_download(self._h, int(row0), int(rows), _ptr(out)))
        return out

    def grid_remove(self, idx1):
        _, d = self.grid_shape()
        row = np.empty(d, dtype=np.float64)
        self._ck(self._L.b7_grid_remove(self._h, int(idx1), _ptr(row)))
        self.grid_version += 1
        return row

    def grid_remove_rows(self, idx1, want_rows=True):
        """Stable deletion of several rows (1-based indices against the grid before the call)."""
        idx = np.ascontiguousarray(np.asarray(idx1, dtype=np.int64).ravel())
        _, d = self.grid_shape()
        rows = np.empty((idx.size, d), dtype=np.float64) if want_rows else None
        self._ck(self._L.b7_grid_remove_rows(self._h, _ptr(idx), idx.size, _ptr(rows)))
        self.grid_version += 1
        return rows

    def grid_colrange(self):
        """grid:min(1), grid:max(1) of the resident grid."""
        _, d = self.grid_shape()
        lo, hi = np.empty(d), np.empty(d)
        self._ck(self._L.b7_grid_colrange(self._h, _ptr(lo), _ptr(hi)))
        return lo, hi

    def grid_apply_onesided(self, mins=None, maxes=None, col_ext=None):
        mn = None if mins is None else _f64(mins).ravel()
        mx = None if maxes is None else _f64(maxes).ravel()
        ext = _f64(col_ext).ravel()
        self._ck(self._L.b7_grid_apply_onesided(self._h, _ptr(mn), _ptr(mx), _ptr(ext)))
        self.grid_version += 1

    def grid_trust_region(self, center, lo, hi, prob, shift=None, seed=0, row_offset=0):
        """The resident grid of base points in [0, 1), mapped in place into a trust-region candidate set (b7_grid_trust_region)."""
        M, d = self.grid_shape()
        vecs = [None if v is None else _f64(v).ravel() for v in (center, lo, hi, shift)]
        if M > 0 and any(v is not None and v.size != d for v in vecs):   # (without a grid the library answers B7_ERR_STATE)
            raise Bot7HipError(-1, "grid_trust_region: center, lo, hi and shift have the grid's %d entries" % d)
        self._ck(self._L.b7_grid_trust_region(self._h, _ptr(vecs[0]), _ptr(vecs[1]), _ptr(vecs[2]), float(prob), _ptr(vecs[3]),
                                              int(seed) & (2 ** 64 - 1), int(row_offset)))
        self.grid_version += 1

    # ---- model
    def gp_set_opts(self, **kw):
        o = GpOpts()
        self._ck(self._L.b7_gp_default_opts(C.byref(o)))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise Bot7HipError(-1, "unknown gp option %r" % k)
            setattr(o, k, v)
        self._ck(self._L.b7_gp_set_opts(self._h, C.byref(o)))

    def gp_set_kernel(self, kernel):
        """The covariance kernel of every later fit, posterior and likelihood: 'ardse' or 'ardmatern52' (or its B7_KERNEL_*
        code).  The library is called only on a change, which drops the fit (fit_token moves: whoever cached "the fit is
        current" refits)."""
        code = kernel_code(kernel)
        if code != self.kernel:
            self._ck(self._L.b7_gp_set_kernel(self._h, code))
            self.kernel = code
            self.fit_token += 1

    def gp_fit(self, X_obs, Y_obs, lenscale_sq, amp, noise, mean, want_nll=False):
        X = _f64(X_obs)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        N, d = X.shape
        Y = _f64(Y_obs).reshape(N, -1)
        ls = _f64(lenscale_sq).ravel()
        if ls.size != d:
            raise Bot7HipError(-1, "lenscale_sq must have d entries")
        hyp = Hyp(ls.ctypes.data_as(C.POINTER(C.c_double)), float(amp), float(noise), float(mean))
        nll = np.empty(Y.shape[1], dtype=np.float64) if want_nll else None
        jit, info = C.c_double(), C.c_int()
        self._ck(self._L.b7_gp_fit(self._h, _ptr(X), _ptr(Y), N, d, Y.shape[1], C.byref(hyp), _ptr(nll),
                                   C.byref(jit), C.byref(info)))
        self.ycols = Y.shape[1]
        self._data_d = d
        self._data_n = N
        self.fit_token += 1
        return {"nll": nll, "jitter": jit.value, "info": info.value}

    def gp_set_data(self, X_obs, Y_obs):
        """Put (X_obs, Y_obs) on the device once; gp_fit_hyp then refits them under new hypers (the sampler's loop)."""
        X = _f64(X_obs)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        N, d = X.shape
        Y = _f64(Y_obs).reshape(N, -1)
        self._ck(self._L.b7_gp_set_data(self._h, _ptr(X), _ptr(Y), N, d, Y.shape[1]))
        self.ycols = Y.shape[1]
        self._data_d = d
        self._data_n = N
        self.fit_token += 1

    def gp_fit_hyp(self, lenscale_sq, amp, noise, mean, want_nll=False):
        ls = _f64(lenscale_sq).ravel()
        if ls.size != getattr(self, "_data_d", -1):
            raise Bot7HipError(-1, "lenscale_sq must have d entries (call gp_set_data first)")
        hyp = Hyp(ls.ctypes.data_as(C.POINTER(C.c_double)), float(amp), float(noise), float(mean))
        nll = np.empty(self.ycols, dtype=np.float64) if want_nll else None
        jit, info = C.c_double(), C.c_int()
        self._ck(self._L.b7_gp_fit_hyp(self._h, C.byref(hyp), _ptr(nll), C.byref(jit), C.byref(info)))
        self.fit_token += 1
        return {"nll": nll, "jitter": jit.value, "info": info.value}

    def gp_predict_hyp(self, lenscale_sq, amp, noise, mean, download=False, want_nll=False):
        """Fit the resident data under the hypers AND predict over the resident grid in one call (no host round trip
        between the two).  Returns the fit report (+ mean, var when download)."""
        ls = _f64(lenscale_sq).ravel()
        if ls.size != getattr(self, "_data_d", -1):
            raise Bot7HipError(-1, "lenscale_sq must have d entries (call gp_set_data first)")
        hyp = Hyp(ls.ctypes.data_as(C.POINTER(C.c_double)), float(amp), float(noise), float(mean))
        nll = np.empty(self.ycols, dtype=np.float64) if want_nll else None
        jit, info = C.c_double(), C.c_int()
        mu = var = None
        if download:
            M, _ = self.grid_shape()
            mu, var = np.empty((M, self.ycols), dtype=np.float64), np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_gp_predict_hyp(self._h, C.byref(hyp), _ptr(mu), _ptr(var), _ptr(nll), C.byref(jit),
                                           C.byref(info)))
        self.fit_token += 1
        out = {"nll": nll, "jitter": jit.value, "info": info.value}
        if download:
            out["mean"], out["var"] = mu, var
        return out

    def gp_nll_batch(self, lenscale_sq, amp, noise, mean, want_info=False):
        """Negative log marginal likelihoods of the resident data (gp_set_data) under B hyper vectors at once."""
        ls = _f64(lenscale_sq)
        ls = ls.reshape(1, -1) if ls.ndim == 1 else ls
        B = ls.shape[0]
        if ls.shape[1] != getattr(self, "_data_d", -1):
            raise Bot7HipError(-1, "lenscale_sq must be B x d (call gp_set_data first)")
        a, nz, m = (np.ascontiguousarray(np.broadcast_to(_f64(v).ravel(), (B,))) for v in (amp, noise, mean))
        nll = np.empty(B, dtype=np.float64)
        jit = np.empty(B, dtype=np.float64)
        info = np.empty(B, dtype=np.int32)
        before = self._L.b7_persist_fallbacks(self._h)
        self._ck(self._L.b7_gp_nll_batch(self._h, B, _ptr(ls), _ptr(a), _ptr(nz), _ptr(m), _ptr(nll), _ptr(jit), _ptr(info)))
        if self._L.b7_persist_fallbacks(self._h) != before:
            self.fit_token += 1      # a timed-out hand-off was redone in the context's fit slot: whoever cached "fit is current" must refit
        return (nll, jit, info) if want_info else nll

    def gp_nll1(self, lenscale_sq, amp, noise, mean):
        """One likelihood evaluation (B = 1) through preallocated argument buffers: what a slice-sampler step costs, without the
        per-call array conversions of gp_nll_batch (the C call itself is ~20-35 us; those conversions were another ~15).
        Returns (nll, jitter, info)."""
        d = getattr(self, "_data_d", -1)
        buf = getattr(self, "_nll1_buf", None)
        if buf is None or buf[0].size != d:
            arr = [np.empty(d), np.empty(1), np.empty(1), np.empty(1), np.empty(1), np.empty(1), np.empty(1, dtype=np.int32)]
            buf = self._nll1_buf = arr + [[_ptr(a) for a in arr]]
        buf[0][:] = lenscale_sq
        buf[1][0], buf[2][0], buf[3][0] = amp, noise, mean
        p = buf[7]
        before = self._L.b7_persist_fallbacks(self._h)
        self._ck(self._L.b7_gp_nll_batch(self._h, 1, p[0], p[1], p[2], p[3], p[4], p[5], p[6]))
        if self._L.b7_persist_fallbacks(self._h) != before:
            self.fit_token += 1
        return float(buf[4][0]), float(buf[5][0]), int(buf[6][0])

    def gp_slice_sample(self, theta0, lo, hi, widths, U, seed, update0=0, max_step=1000, max_evals=512, gibbs=False,
                        logspace=True):
        """C slice-sampling chains of U updates over the resident data in ONE launch (b7_gp_slice_sample): theta0 is C x (d + 3)
        (or one start point), theta = [log lenscale_sq, log amp, log noise, mean]; lo, hi, widths have d + 3 entries.  Returns
        {'theta': C x U x (d + 3), 'value': C x U, 'status': C x U bit masks (SLICE_*), 'nevals': C}.  The kernel runs the
        sampler's default mode only: Gibbs updates and linear space are refused by name."""
        if gibbs:
            raise Bot7HipError(-5, "gp_slice_sample: Gibbs updates are not built on the device (random direction only)")
        if not logspace:
            raise Bot7HipError(-5, "gp_slice_sample: linear space is not built on the device (log space only)")
        D = getattr(self, "_data_d", -4) + 3
        t0 = _f64(theta0)
        t0 = t0.reshape(1, -1) if t0.ndim == 1 else t0
        lo, hi, wd = _f64(lo).ravel(), _f64(hi).ravel(), _f64(widths).ravel()
        if D >= 4 and (t0.shape[1] != D or lo.size != D or hi.size != D or wd.size != D):
            raise Bot7HipError(-1, "gp_slice_sample: theta0 must be C x (d + 3), lo / hi / widths d + 3 long")
        Cn, U = t0.shape[0], int(U)
        D = t0.shape[1]
        n = max(Cn, 0) * max(U, 0)
        theta = np.empty((Cn, max(U, 0), D), dtype=np.float64)
        value = np.empty((Cn, max(U, 0)), dtype=np.float64)
        status = np.empty((Cn, max(U, 0)), dtype=np.int32)
        nev = np.empty(max(Cn, 1), dtype=np.int32)
        keep = [np.empty(max(n, 1))]  # (a zero-sized array has no address worth passing)
        self._ck(self._L.b7_gp_slice_sample(self._h, Cn, U, _ptr(t0), _ptr(lo), _ptr(hi), _ptr(wd), int(max_step), int(max_evals),
                                            int(seed) & (2 ** 64 - 1), int(update0) & (2 ** 64 - 1),
                                            _ptr(theta if n else keep[0]), _ptr(value if n else keep[0]),
                                            _ptr(status if n else keep[0]), _ptr(nev)))
        self._slice_shape = (Cn, D)
        return {"theta": theta, "value": value, "status": status, "nevals": nev[:Cn]}

    def gp_slice_trace_enable(self, records_per_chain):
        """Keep the first `records_per_chain` trace records of every chain of the following gp_slice_sample calls (0: off)."""
        self._ck(self._L.b7_gp_slice_trace_enable(self._h, int(records_per_chain)))
        self._slice_rpc = int(records_per_chain)

    def gp_slice_trace(self, chain):
        """Chain `chain`'s records of the last traced gp_slice_sample, in order, as a list of dicts: an update's draws
        {'type': 'update', 'g', 'u_Y', 'log_u_Y', 'z', 'u_right'} or a density request {'type': 'request', 'kind' (0 start,
        1 step-out right, 2 step-out left, 3 shrink), 'u', 'in_bounds', 'reused', 'value', 'ticks' (100 MHz), 'theta', 'hyp'}."""
        rpc = getattr(self, "_slice_rpc", 0)
        D = getattr(self, "_slice_shape", (0, 0))[1]
        buf = np.zeros((max(rpc, 1), SLICE_TRACE_WIDTH), dtype=np.float64)
        n = C.c_int()
        self._ck(self._L.b7_gp_slice_trace(self._h, int(chain), _ptr(buf), C.byref(n)))
        out = []
        for r in buf[:n.value]:
            if r[0] == 0.0:
                out.append({"type": "update", "g": int(r[1]), "u_Y": r[2], "log_u_Y": r[3], "z": r[8:8 + D].copy(),
                            "u_right": r[72:72 + D].copy()})
            else:
                out.append({"type": "request", "kind": int(r[1]), "u": r[2], "in_bounds": bool(r[3]), "reused": bool(r[4]),
                            "value": r[5], "ticks": r[6], "theta": r[8:8 + D].copy(), "hyp": r[72:72 + D].copy()})
        return out

    def chol(self, src):
        """utils.math.chol(src, 'L') with the jitter schedule; returns (L, jitter_used, info_first)."""
        A = _f64(src)
        n = A.shape[0]
        res = np.empty((n, n), dtype=np.float64)
        jit, info = C.c_double(), C.c_int()
        self._ck(self._L.b7_chol(self._h, _ptr(A), n, _ptr(res), C.byref(jit), C.byref(info)))
        self.fit_token += 1
        return res, jit.value, info.value

    def gp_predict(self, download=True):
        M, _ = self.grid_shape()
        if not download:
            self._ck(self._L.b7_gp_predict(self._h, None, None))
            return None, None
        mean = np.empty((M, getattr(self, "ycols", 1)), dtype=np.float64)
        var = np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_gp_predict(self._h, _ptr(mean), _ptr(var)))
        return mean, var

    def gp_predict_at(self, X1):
        X1 = _f64(X1)
        if X1.ndim == 1:
            X1 = X1.reshape(1, -1)
        mean = np.empty((X1.shape[0], getattr(self, "ycols", 1)), dtype=np.float64)
        var = np.empty(X1.shape[0], dtype=np.float64)
        self._ck(self._L.b7_gp_predict_at(self._h, _ptr(X1), X1.shape[0], _ptr(mean), _ptr(var)))
        return mean, var

    def gp_fantasize(self, X_pend, nFantasies, seed=0, want_moments=False):
        """nFantasies joint posterior draws at the pending points: P x nFantasies (+ mu_P, Sigma_P).  A draw depends on
        nFantasies as well as on the seed: z(k, s) = counter_normal(seed, k * nFantasies + s)."""
        Xp = _f64(X_pend)
        if Xp.ndim == 1:
            Xp = Xp.reshape(1, -1)
        P = Xp.shape[0]
        out = np.empty((P, int(nFantasies)), dtype=np.float64)
        mu = np.empty(P, dtype=np.float64) if want_moments else None
        cov = np.empty((P, P), dtype=np.float64) if want_moments else None
        self._ck(self._L.b7_gp_fantasize(self._h, _ptr(Xp), P, int(nFantasies), int(seed) & (2 ** 64 - 1), _ptr(out),
                                         _ptr(mu), _ptr(cov)))
        return (out, mu, cov) if want_moments else out

    def gp_append(self, x_new, y_new):
        """Extend the current fit by one observation under the same hypers (O(N^2))."""
        x = _f64(x_new).ravel()
        y = _f64(y_new).ravel()
        self._ck(self._L.b7_gp_append(self._h, _ptr(x), _ptr(y)))
        if hasattr(self, "_data_n"):
            self._data_n += 1

    def gp_download(self, N, ycols=1):
        Lh = np.empty((N, N), dtype=np.float64)
        al = np.empty((N, ycols), dtype=np.float64)
        Li = np.empty((N, N), dtype=np.float64)
        self._ck(self._L.b7_gp_download(self._h, _ptr(Lh), _ptr(al), _ptr(Li)))
        return Lh, al, Li

    # ---- DNGO: basis network + Bayesian linear head
    @staticmethod
    def _mlp(weights, biases, activation):
        Ws = [_f64(w) for w in weights]
        bs = [_f64(b).ravel() for b in biases]
        # the same arrays as last time (a trial loop hands the same network to every call until it retrains it): the ctypes
        # description is reused -- it only holds pointers, the library reads the weights themselves on every call
        key = (activation,) + tuple((w.__array_interface__["data"][0], w.shape) for w in Ws) + tuple(
            (b.__array_interface__["data"][0], b.shape) for b in bs)
        hit = _MLP_CACHE.get(key)
        if hit is not None:
            return hit
        n = len(Ws)
        dims = (C.c_int * (n + 1))(*([Ws[0].shape[1]] + [w.shape[0] for w in Ws]))
        Wp = (C.POINTER(C.c_double) * n)(*[w.ctypes.data_as(C.POINTER(C.c_double)) for w in Ws])
        bp = (C.POINTER(C.c_double) * n)(*[b.ctypes.data_as(C.POINTER(C.c_double)) for b in bs])
        m = Mlp(n, dims, Wp, bp, ACTIVATIONS[activation])
        m._keep = (Ws, bs, dims, Wp, bp)      # the arrays stay alive as long as the description does
        if len(_MLP_CACHE) >= 8:
            _MLP_CACHE.clear()
        _MLP_CACHE[key] = m
        return m

    def blr_basis(self, weights, biases, activation="Tanh", X=None, download=False):
        """Features of X (host rows) or, with X=None, of the resident grid (kept on the device)."""
        net = self._mlp(weights, biases, activation)
        z = net._keep[0][-1].shape[0]
        if X is None:
            M, _ = self.grid_shape()
            out = np.empty((M, z), dtype=np.float64) if download else None
            self._ck(self._L.b7_blr_basis(self._h, C.byref(net), None, 0, _ptr(out)))
            return out
        X = _f64(X)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        out = np.empty((X.shape[0], z), dtype=np.float64)
        self._ck(self._L.b7_blr_basis(self._h, C.byref(net), _ptr(X), X.shape[0], _ptr(out)))
        return out

    def blr_features(self, Z1):
        Z1 = _f64(Z1)
        self._ck(self._L.b7_blr_features(self._h, _ptr(Z1), Z1.shape[0], Z1.shape[1]))
        self.grid_version += 1

    def blr_fit(self, Z0, Y0, alpha_prec, beta, mean=0.0, want_nll=False):
        Z0 = _f64(Z0)
        Y0 = _f64(Y0).ravel()
        nll = C.c_double()
        self._ck(self._L.b7_blr_fit(self._h, _ptr(Z0), _ptr(Y0), Z0.shape[0], Z0.shape[1], float(alpha_prec),
                                    float(beta), float(mean), C.byref(nll) if want_nll else None))
        self.ycols = 1
        self.fit_token += 1
        return nll.value if want_nll else None

    def blr_fit_x(self, weights, biases, activation, X0, Y0, alpha_prec, beta, mean=0.0, want_nll=False):
        """Basis features of X0 and the Bayesian-linear fit in one device-side call."""
        net = self._mlp(weights, biases, activation)
        X0 = _f64(X0)
        Y0 = _f64(Y0).ravel()
        nll = C.c_double()
        self._ck(self._L.b7_blr_fit_x(self._h, C.byref(net), _ptr(X0), _ptr(Y0), X0.shape[0], float(alpha_prec),
                                      float(beta), float(mean), C.byref(nll) if want_nll else None))
        self.ycols = 1
        self.fit_token += 1
        return nll.value if want_nll else None

    def blr_eval_nominate(self, weights, biases, activation, X0, Y0, alpha_prec, beta, mean=0.0, score="ei", fmin=None,
                          tradeoff=None, upper=False, sign=-1.0, global_row_offset=0, want_jitter=False):
        """bayesopt:eval's DNGO branch + nominate in one call -> (value, 1-based global index[, jitter flag])."""
        net = self._mlp(weights, biases, activation)
        X0 = _f64(X0)
        Y0 = _f64(Y0).ravel()
        spec, fm = self._pack_spec(score, fmin, tradeoff, upper, sign)
        v, i, j = C.c_double(), C.c_int64(), C.c_double()
        self._ck(self._L.b7_blr_eval_nominate(self._h, C.byref(net), _ptr(X0), _ptr(Y0), X0.shape[0], float(alpha_prec),
                                              float(beta), float(mean), C.byref(spec), int(global_row_offset), C.byref(v),
                                              C.byref(i), C.byref(j)))
        self.fit_token += 1
        return (v.value, i.value, j.value) if want_jitter else (v.value, i.value)

    def blr_eval_nominate_marg(self, weights, biases, activation, X0, Y0, alphas, betas, means, score="ei", fmin=None,
                               tradeoff=None, upper=False, sign=-1.0, global_row_offset=0, want_nll=False):
        """bayesopt:eval's DNGO branch with the head's hypers marginalised (models/dngo.lua:109,174): S samples (alpha, beta, mean),
        S heads over the same features, score:add per sample, score:div(S), score:max(1).  Returns (value, 1-based global index,
        jitter flag[, nll per sample])."""
        net = self._mlp(weights, biases, activation)
        X = _f64(X0)
        Y = _f64(Y0).ravel()
        a, b, m = (np.ascontiguousarray(_f64(v).ravel()) for v in (alphas, betas, means))
        S = a.size
        if b.size != S or m.size != S:
            raise Bot7HipError(-1, "alphas, betas and means must have the same length")
        spec, fm = self._pack_spec(score, fmin, tradeoff, upper, sign)
        nll = np.empty(S, dtype=np.float64) if want_nll else None
        v, i, jit = C.c_double(), C.c_int64(), C.c_double()
        self._ck(self._L.b7_blr_eval_nominate_marg(self._h, C.byref(net), _ptr(X), _ptr(Y), X.shape[0], S, _ptr(a), _ptr(b), _ptr(m),
                                                   C.byref(spec), int(global_row_offset), C.byref(v), C.byref(i), _ptr(nll),
                                                   C.byref(jit)))
        self.fit_token += 1
        return (v.value, i.value, jit.value, nll) if want_nll else (v.value, i.value, jit.value)

    def blr_predict(self, download=True):
        M, _ = self.grid_shape()
        if not download:
            self._ck(self._L.b7_blr_predict(self._h, None, None))
            return None, None
        mean = np.empty((M, 1), dtype=np.float64)
        var = np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_blr_predict(self._h, _ptr(mean), _ptr(var)))
        return mean, var

    # ---- scores
    def score_reset(self):
        self._ck(self._L.b7_score_reset(self._h))

    def score_ei(self, fmin, tradeoff=0.0):
        f = _f64(fmin).ravel()
        self._ck(self._L.b7_score_ei(self._h, _ptr(f), float(tradeoff)))

    def score_logei(self, fmin, tradeoff=0.0):
        """Log-space EI of the last predict, folded into the accumulator as a running log-sum-exp (b7_score_logei)."""
        f = _f64(fmin).ravel()
        self._ck(self._L.b7_score_logei(self._h, _ptr(f), float(tradeoff)))

    def score_logpi(self, fmin, tradeoff=0.0):
        """Log probability of improvement of the last predict, log Phi(z), folded into the accumulator as a running log-sum-exp
        (b7_score_logpi).  With fmin = a constraint's threshold and tradeoff = 0 on that constraint's GP: its log probability of
        feasibility."""
        f = _f64(fmin).ravel()
        self._ck(self._L.b7_score_logpi(self._h, _ptr(f), float(tradeoff)))

    def score_mes(self):
        """Max-value entropy search of the last predict: the y* search on the device, then score:add (b7_score_mes)."""
        self._ck(self._L.b7_score_mes(self._h))

    def mes_set_levels(self, K):
        """K quantiles of the grid minimum per hyper sample for the searches that follow (b7_mes_set_levels; default 8)."""
        self._ck(self._L.b7_mes_set_levels(self._h, int(K)))

    def mes_last_ystar(self):
        """(ystar S x K, bracket S x 2 = lo0, hi0) of the last y* search on this context (b7_mes_last_ystar)."""
        S, K = C.c_int(0), C.c_int(0)
        self._ck(self._L.b7_mes_last_ystar(self._h, C.byref(S), C.byref(K), None, None))
        ystar, bracket = np.empty((S.value, K.value), dtype=np.float64), np.empty((S.value, 2), dtype=np.float64)
        self._ck(self._L.b7_mes_last_ystar(self._h, None, None, _ptr(ystar), _ptr(bracket)))
        return ystar, bracket

    def mes_ystar(self, mean, var, K=8):
        """The y* search alone on caller-provided mean / var (M each): (ystar K, bracket 2 = lo0, hi0) (b7_mes_ystar)."""
        mean, var = _f64(mean).ravel(), _f64(var).ravel()
        ystar, bracket = np.empty(int(K) if 1 <= int(K) <= MES_KMAX else 1, dtype=np.float64), np.empty(2, dtype=np.float64)
        self._ck(self._L.b7_mes_ystar(self._h, _ptr(mean), _ptr(var), mean.shape[0], int(K), _ptr(ystar), _ptr(bracket)))
        return ystar, bracket

    def mes_compute(self, mean, var, ystar):
        """The MES score on caller-provided mean / var (M each) with the caller's y* (K values) (b7_mes_compute)."""
        mean, var, ystar = _f64(mean).ravel(), _f64(var).ravel(), _f64(ystar).ravel()
        out = np.empty(mean.shape[0], dtype=np.float64)
        self._ck(self._L.b7_mes_compute(self._h, _ptr(mean), _ptr(var), _ptr(ystar), ystar.shape[0], mean.shape[0], _ptr(out)))
        return out

    def score_cb(self, tradeoff=1.0, upper=False, sign=-1.0):
        self._ck(self._L.b7_score_cb(self._h, float(tradeoff), int(bool(upper)), float(sign)))

    def score_finish(self, divisor=1.0, download=False):
        v, i = C.c_double(), C.c_int64()
        out = None
        if download:
            M, _ = self.grid_shape()
            out = np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_score_finish(self._h, float(divisor), C.byref(v), C.byref(i), _ptr(out)))
        return v.value, i.value, out

    # ---- multi-GPU: the arg-max exchange over RCCL (one process per GPU, one context each)
    def comm_init(self, rank, world, id_bytes):
        """ncclCommInitRank on this context's GPU; id_bytes = comm_unique_id() of rank 0 (collective call)."""
        buf = C.create_string_buffer(bytes(id_bytes), COMM_ID_BYTES)
        self._ck(self._L.b7_comm_init(self._h, int(rank), int(world), C.cast(buf, C.c_void_p)))

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        self._ck(self._L.b7_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_destroy(self):
        self._ck(self._L.b7_comm_destroy(self._h))

    def comm_allreduce(self, values, op="sum"):
        """A few host doubles reduced over the communicator (control plane; doubles as a barrier)."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel()).copy()
        self._ck(self._L.b7_comm_allreduce_f64(self._h, _ptr(v), v.size, {"sum": 0, "max": 1, "min": 2}[op]))
        return v

    def score_finish_global(self, divisor=1.0, global_row_offset=0):
        """score:div + score:max(1) over the candidates of ALL ranks -> (value, 1-based global index)."""
        v, i = C.c_double(), C.c_int64()
        self._ck(self._L.b7_score_finish_global(self._h, float(divisor), int(global_row_offset), C.byref(v),
                                                C.byref(i)))
        return v.value, i.value

    def nominate_commit(self, idx1_global, global_row_offset=0):
        """bots/abstract.lua:118 on a sharded candidate set -> (nominee's row, this rank's new row offset)."""
        _, d = self.grid_shape()
        row, off = np.empty(d, dtype=np.float64), C.c_int64(int(global_row_offset))
        self._ck(self._L.b7_nominate_commit(self._h, int(idx1_global), C.byref(off), _ptr(row)))
        self.grid_version += 1
        return row, off.value

    def exchange_info(self):
        """The last exchange as this rank saw it: rows per rank, winner index / rank / row."""
        w, wi, wr = C.c_int(), C.c_int64(), C.c_int()
        rows, row = np.zeros(64, dtype=np.int64), np.zeros(96, dtype=np.float64)
        self._ck(self._L.b7_exchange_info(self._h, C.byref(w), _ptr(rows), C.byref(wi), C.byref(wr), _ptr(row)))
        _, d = self.grid_shape()
        return {"world": w.value, "rows": rows[:w.value].copy(), "winner_idx1": wi.value, "winner_rank": wr.value,
                "winner_row": row[:d].copy()}

    @staticmethod
    def _pack_hyps(hyps, d):
        S = len(hyps)
        arr = (Hyp * S)()
        keep = []
        for s, h in enumerate(hyps):
            if isinstance(h, dict):
                h = (h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
            ls = _f64(h[0]).ravel()
            if ls.size != d:
                raise Bot7HipError(-1, "lenscale_sq must have d entries (call gp_set_data first)")
            keep.append(ls)
            arr[s] = Hyp(ls.ctypes.data_as(C.POINTER(C.c_double)), float(h[1]), float(h[2]), float(h[3]))
        return arr, keep

    @staticmethod
    def _pack_spec(score, fmin, tradeoff, upper, sign):
        if score in _FMIN_SCORES:
            if fmin is None:
                raise Bot7HipError(-1, "%s needs fmin" % ("LogPI" if score == "logpi" else "EI"))
            fm = _f64(fmin).ravel()
            return ScoreSpec(_FMIN_SCORES[score], 0.0 if tradeoff is None else float(tradeoff), 0, 0.0,
                             fm.ctypes.data_as(C.POINTER(C.c_double))), fm
        if score == "mes":  # fmin, tradeoff, upper and sign are ignored
            return ScoreSpec(SCORE_MES, 0.0, 0, 0.0, None), None
        if score == "cb":
            return ScoreSpec(SCORE_CB, 1.0 if tradeoff is None else float(tradeoff), int(bool(upper)), float(sign),
                             None), None
        raise Bot7HipError(-1, "score must be 'ei', 'logei', 'logpi', 'mes' or 'cb'")

    def eval_nominate(self, hyps, score="ei", fmin=None, tradeoff=None, upper=False, sign=-1.0,
                      global_row_offset=0, want_report=False, levels=None):
        """bayesopt:eval + nominate in one call: hyps is a sequence of (lenscale_sq, amp, noise, mean) or dicts
        with those keys; score "ei" / "logei" / "logpi" (need fmin), "cb" or "mes" (levels: mes_set_levels first).  Returns (value, 1-based
        global index[, report])."""
        if levels is not None:
            self.mes_set_levels(levels)
        S = len(hyps)
        arr, keep = self._pack_hyps(hyps, getattr(self, "_data_d", -1))
        spec, fm = self._pack_spec(score, fmin, tradeoff, upper, sign)
        jit = np.zeros(S, dtype=np.float64) if want_report else None
        info = np.zeros(S, dtype=np.int32) if want_report else None
        v, i = C.c_double(), C.c_int64()
        self._ck(self._L.b7_eval_nominate(self._h, S, arr, C.byref(spec), int(global_row_offset), C.byref(v),
                                          C.byref(i), _ptr(jit), _ptr(info)))
        self.fit_token += 1
        if want_report:
            return v.value, i.value, {"jitter": jit, "info": info}
        return v.value, i.value

    # ---- constrained nomination: the feasibility column (log-weights over the resident grid) and the weighted arg-max
    def feas_reset(self):
        """L := 0.0 over the resident grid (b7_feas_reset).  Any change of the grid forgets the column."""
        self._ck(self._L.b7_feas_reset(self._h))

    def feas_add(self, logw):
        """L[j] += logw[j] from a host vector with one entry per grid row; -inf masks a row (b7_feas_add)."""
        w = _f64(logw).ravel()
        self._ck(self._L.b7_feas_add(self._h, _ptr(w), w.size))

    def feas_add_acc(self, src):
        """L[j] += the accumulator of the context `src`, device to device: what src.eval_nominate(score="logpi") leaves, the
        marginal log probability already divided (b7_feas_add_acc).  Both contexts must hold the same grid rows: the caller's
        contract, only the row count is checked."""
        if not isinstance(src, Context) or src._L is not self._L:
            raise Bot7HipError(-1, "feas_add_acc: src must be a Context of the same library")
        self._ck(self._L.b7_feas_add_acc(self._h, src._h))

    def feas_get(self):
        """The column L, one entry per grid row (b7_feas_get)."""
        M, _ = self.grid_shape()
        out = np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_feas_get(self._h, _ptr(out)))
        return out

    def feas_nominate(self):
        """score:max(1) of the column alone -> (value, 1-based index): the nomination while no feasible observation exists
        (b7_feas_nominate).  The column is left untouched."""
        v, i = C.c_double(), C.c_int64()
        self._ck(self._L.b7_feas_nominate(self._h, C.byref(v), C.byref(i)))
        return v.value, i.value

    def eval_nominate_feasible(self, hyps, score="logei", fmin=None, tradeoff=None, upper=False, sign=-1.0, want_report=False):
        """eval_nominate with the feasibility column weighted in between score:div and score:max(1): score + L for the log kinds
        ("logei", "logpi"), score * exp(L) for "ei" (b7_eval_nominate_feasible; "cb" and "mes" reach the library, which answers
        "unsupported").  Returns (value, 1-based index[, report]); the accumulator holds the weighted score afterwards."""
        S = len(hyps)
        arr, keep = self._pack_hyps(hyps, getattr(self, "_data_d", -1))
        spec, fm = self._pack_spec(score, fmin, tradeoff, upper, sign)
        jit = np.zeros(S, dtype=np.float64) if want_report else None
        info = np.zeros(S, dtype=np.int32) if want_report else None
        v, i = C.c_double(), C.c_int64()
        self._ck(self._L.b7_eval_nominate_feasible(self._h, S, arr, C.byref(spec), C.byref(v), C.byref(i), _ptr(jit), _ptr(info)))
        self.fit_token += 1
        if want_report:
            return v.value, i.value, {"jitter": jit, "info": info}
        return v.value, i.value

    def eval_nominate_batch(self, hyps, q, score="ei", fmin=None, tradeoff=None, upper=False, sign=-1.0, want_report=False, levels=None):
        """A greedy batch of q nominees (b7_eval_nominate_batch): eval_nominate's pick, then q - 1 more by kriging-believer
        variance downdates, the rows already picked left out.  hyps, score, fmin, tradeoff, upper, sign, levels as eval_nominate
        (score "mes" reaches the library, which answers "unsupported" for batches).
        Returns (values[q], 1-based indices[q][, report]); the grid is not modified (commit with grid_remove_rows)."""
        if levels is not None:
            self.mes_set_levels(levels)
        S = len(hyps)
        arr, keep = self._pack_hyps(hyps, getattr(self, "_data_d", -1))
        spec, fm = self._pack_spec(score, fmin, tradeoff, upper, sign)
        jit = np.zeros(S, dtype=np.float64) if want_report else None
        info = np.zeros(S, dtype=np.int32) if want_report else None
        n = max(int(q), 1)
        vals, idx = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64)
        self._ck(self._L.b7_eval_nominate_batch(self._h, S, arr, C.byref(spec), int(q), _ptr(vals), _ptr(idx), _ptr(jit), _ptr(info)))
        self.fit_token += 1
        if want_report:
            return vals, idx, {"jitter": jit, "info": info}
        return vals, idx

    def eval_nominate_refine(self, hyps, score="ei", fmin=None, tradeoff=None, upper=False, sign=-1.0, starts=16, iters=16,
                             eta0=1.0 / 16.0, lo=None, hi=None, want_report=False):
        """eval_nominate, then the nominee refined off the grid by gradient ascent on the marginalised acquisition from `starts`
        starts for `iters` iterations inside the box [lo, hi] (None: the unit cube) (b7_eval_nominate_refine).  hyps, score, fmin,
        tradeoff, upper, sign as eval_nominate (score "mes" reaches the library, which answers "unsupported").
        Returns (value, 1-based index, x[d], refined value, 1-based index of the winner's start[, report]); the grid is not modified."""
        S = len(hyps)
        d = getattr(self, "_data_d", -1)
        arr, keep = self._pack_hyps(hyps, d)
        spec, fm = self._pack_spec(score, fmin, tradeoff, upper, sign)
        lo = None if lo is None else _f64(lo).ravel()
        hi = None if hi is None else _f64(hi).ravel()
        for b in (lo, hi):
            if b is not None and b.size != d:
                raise Bot7HipError(-1, "lo / hi must have d entries")
        dp = C.POINTER(C.c_double)
        opts = RefineOpts(int(starts), int(iters), float(eta0), None if lo is None else lo.ctypes.data_as(dp),
                          None if hi is None else hi.ctypes.data_as(dp))
        jit = np.zeros(S, dtype=np.float64) if want_report else None
        info = np.zeros(S, dtype=np.int32) if want_report else None
        v, i, rv, ri = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        x = np.zeros(max(d, 1), dtype=np.float64)
        self._ck(self._L.b7_eval_nominate_refine(self._h, S, arr, C.byref(spec), C.byref(opts), C.byref(v), C.byref(i), _ptr(x),
                                                 C.byref(rv), C.byref(ri), _ptr(jit), _ptr(info)))
        self.fit_token += 1
        if want_report:
            return v.value, i.value, x, rv.value, ri.value, {"jitter": jit, "info": info}
        return v.value, i.value, x, rv.value, ri.value

    def refine_last(self):
        """Every start of the last eval_nominate_refine: dict(x P x d, val P, start_idx1 P, status P) (b7_refine_last)."""
        P, d, _, _ = self.refine_shape()
        n = C.c_int()
        x, val = np.zeros((REFINE_MAX_STARTS, d), dtype=np.float64), np.zeros(REFINE_MAX_STARTS, dtype=np.float64)
        idx, status = np.zeros(REFINE_MAX_STARTS, dtype=np.int64), np.zeros(REFINE_MAX_STARTS, dtype=np.int32)
        self._ck(self._L.b7_refine_last(self._h, C.byref(n), _ptr(x), _ptr(val), _ptr(idx), _ptr(status)))
        P = n.value
        return {"x": x[:P].copy(), "val": val[:P].copy(), "start_idx1": idx[:P].copy(), "status": status[:P].copy()}

    def refine_shape(self):
        """(starts, d, iters, traced) of the last eval_nominate_refine, from the library (b7_refine_shape)."""
        P, d, it, tr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.b7_refine_shape(self._h, C.byref(P), C.byref(d), C.byref(it), C.byref(tr)))
        return P.value, d.value, it.value, bool(tr.value)

    def refine_trace_enable(self, on=True):
        """Keep one record per start and iteration of the eval_nominate_refine calls that follow (b7_refine_trace_enable)."""
        self._ck(self._L.b7_refine_trace_enable(self._h, int(bool(on))))

    def refine_trace(self, start):
        """Start `start`'s records of the last traced eval_nominate_refine, iteration 0..iters, as a dict of arrays: x (n x d, the
        point after the iteration), val, grad (n x d), eta (before the step), cand (n x 4, NaN where no ladder ran), rung (-1:
        stayed), status (b7_refine_trace)."""
        _, d, iters, _ = self.refine_shape()
        buf = np.zeros((iters + 1, REFINE_TRACE_WIDTH), dtype=np.float64)
        n = C.c_int()
        self._ck(self._L.b7_refine_trace(self._h, int(start), _ptr(buf), C.byref(n)))
        r = buf[:n.value]
        return {"x": r[:, :d].copy(), "val": r[:, d].copy(), "grad": r[:, d + 1:2 * d + 1].copy(), "eta": r[:, 2 * d + 1].copy(),
                "cand": r[:, 2 * d + 2:2 * d + 6].copy(), "rung": r[:, 2 * d + 6].astype(np.int64),
                "status": r[:, 2 * d + 7].astype(np.int64)}

    def gp_grad_at(self, X1):
        """The current fit's posterior at the rows of X1 with gradients: (mean M1, var M1, dmean M1 x d, dvar M1 x d); var is the
        latent variance (b7_gp_grad_at)."""
        X1 = _f64(X1)
        if X1.ndim == 1:
            X1 = X1.reshape(1, -1)
        M1, d = X1.shape
        mean, var = np.empty(M1, dtype=np.float64), np.empty(M1, dtype=np.float64)
        dmean, dvar = np.empty((M1, d), dtype=np.float64), np.empty((M1, d), dtype=np.float64)
        self._ck(self._L.b7_gp_grad_at(self._h, _ptr(X1), M1, _ptr(mean), _ptr(var), _ptr(dmean), _ptr(dvar)))
        return mean, var, dmean, dvar

    def score_grad_compute(self, mean, var, dmean, dvar, score="ei", fmin=None, tradeoff=None, upper=False, sign=-1.0):
        """The marginal score and its gradient from S samples' mean / var (S x M1) and their gradients (S x M1 x d) on host
        arrays -> (value M1, grad M1 x d) (b7_score_grad_compute)."""
        dmean, dvar = _f64(dmean), _f64(dvar)
        if dmean.ndim == 2:
            dmean, dvar = dmean[None], dvar[None]
        S, M1, d = dmean.shape
        mean, var = _f64(mean).reshape(S, M1), _f64(var).reshape(S, M1)
        dvar = dvar.reshape(S, M1, d)
        spec, fm = self._pack_spec(score, fmin, tradeoff, upper, sign)
        value, grad = np.empty(M1, dtype=np.float64), np.empty((M1, d), dtype=np.float64)
        self._ck(self._L.b7_score_grad_compute(self._h, C.byref(spec), S, _ptr(mean), _ptr(var), _ptr(dmean), _ptr(dvar), M1, d,
                                               _ptr(value), _ptr(grad)))
        return value, grad

    def ts_nominate(self, hyps, q, n_features=1024, seed=0, want_report=False):
        """Thompson sampling (b7_ts_nominate): q pathwise posterior samples over the resident data and grid, path j under hyper
        sample j mod len(hyps), each path's first minimum among the rows no earlier path of the call took.
        Returns (path minima[q], 1-based indices[q][, report]); the grid is not modified (commit with grid_remove_rows)."""
        S = len(hyps)
        arr, keep = self._pack_hyps(hyps, getattr(self, "_data_d", -1))
        jit = np.zeros(max(S, 1), dtype=np.float64) if want_report else None
        info = np.zeros(max(S, 1), dtype=np.int32) if want_report else None
        n = max(int(q), 1)
        vals, idx = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64)
        self._ck(self._L.b7_ts_nominate(self._h, S, arr, int(q), int(n_features), int(seed) & (2 ** 64 - 1), _ptr(vals), _ptr(idx),
                                        _ptr(jit), _ptr(info)))
        self.fit_token += 1
        self._ts_shape = (self.grid_shape()[0], n, int(n_features), self._data_d, getattr(self, "_data_n", 0))   # what the inspection entries return
        if want_report:
            return vals, idx, {"jitter": jit[:S], "info": info[:S]}
        return vals, idx

    def ts_last_paths(self):
        """The last ts_nominate's sample paths over the grid as it stood, M x q (b7_ts_last_paths)."""
        M, q = getattr(self, "_ts_shape", (1, 1, 0, 0, 0))[:2]
        out = np.empty((M, q), dtype=np.float64)
        self._ck(self._L.b7_ts_last_paths(self._h, _ptr(out)))
        return out

    def ts_last_draws(self, path):
        """Path `path`'s draws of the last ts_nominate: dict(omega F x d, phase F, weight F, eps N) (b7_ts_last_draws)."""
        _, _, F, d, N = getattr(self, "_ts_shape", (1, 1, 1, 1, 1))
        out = {"omega": np.empty((F, d), dtype=np.float64), "phase": np.empty(F, dtype=np.float64),
               "weight": np.empty(F, dtype=np.float64), "eps": np.empty(N, dtype=np.float64)}
        self._ck(self._L.b7_ts_last_draws(self._h, int(path), _ptr(out["omega"]), _ptr(out["phase"]), _ptr(out["weight"]), _ptr(out["eps"])))
        return out

    def kg_nominate(self, hyps, points=KG_MAX_POINTS, rows=None, want_report=False, trace=False):
        """The knowledge gradient (b7_kg_nominate): the row of the resident grid whose evaluation is expected to lower the minimum of
        the posterior mean the most, marginalised over hyps.  points: the size n of the discretisation set (1..KG_MAX_POINTS);
        rows: its n distinct 1-based grid rows (None: the library takes the n rows of lowest marginal mean).  trace: keep the
        slopes for kg_last.  Returns (value, 1-based index[, report]); the grid is not modified."""
        S = len(hyps)
        arr, keep = self._pack_hyps(hyps, getattr(self, "_data_d", -1))
        rows1 = None
        if rows is not None:
            rows1 = np.ascontiguousarray(np.asarray(rows).ravel(), dtype=np.int64)
            points = rows1.size
        jit = np.zeros(max(S, 1), dtype=np.float64) if want_report else None
        info = np.zeros(max(S, 1), dtype=np.int32) if want_report else None
        val, idx = C.c_double(), C.c_int64()
        self._ck(self._L.b7_kg_trace_enable(self._h, 1 if trace else 0))
        self._ck(self._L.b7_kg_nominate(self._h, S, arr, int(points), _ptr(rows1), C.byref(val), C.byref(idx), _ptr(jit), _ptr(info)))
        self.fit_token += 1
        self._kg_shape = (S, self.grid_shape()[0], int(points))   # what kg_last returns
        if want_report:
            return val.value, idx.value, {"jitter": jit[:S], "info": info[:S]}
        return val.value, idx.value

    def kg_last(self, slopes=False):
        """What the last kg_nominate used and made (b7_kg_last): dict(rows n (1-based), alpha S x n, values S x M, own_alpha S x M[,
        slopes S x M x (n + 1): column 0 the own line, NaN where the row is in the discretisation set]); slopes needs trace=True."""
        S, M, n = getattr(self, "_kg_shape", (1, 1, 1))
        out = {"rows": np.zeros(n, dtype=np.int64), "alpha": np.empty((S, n), dtype=np.float64),
               "values": np.empty((S, M), dtype=np.float64), "own_alpha": np.empty((S, M), dtype=np.float64)}
        if slopes:
            out["slopes"] = np.empty((S, M, n + 1), dtype=np.float64)
        self._ck(self._L.b7_kg_last(self._h, _ptr(out["rows"]), _ptr(out["alpha"]), _ptr(out.get("slopes")), _ptr(out["values"]),
                                    _ptr(out["own_alpha"])))
        return out

    def kg_compute(self, alpha, b):
        """min_i alpha_i - E[min_i (alpha_i + b_i Z)] per row of alpha, b (M1 x L, L <= KG_MAX_POINTS + 1) by the nomination's own
        code (b7_kg_compute); column 0 is the own line, a NaN slope there means the row has none."""
        alpha, b = _f64(alpha), _f64(b)
        if alpha.ndim != 2 or alpha.shape != b.shape:
            raise Bot7HipError(-1, "kg_compute: alpha and b are M1 x L")
        out = np.empty(alpha.shape[0], dtype=np.float64)
        self._ck(self._L.b7_kg_compute(self._h, alpha.shape[0], alpha.shape[1], _ptr(alpha), _ptr(b), _ptr(out)))
        return out

    # ---- two objectives: the kept posterior and the expected hypervolume improvement (csrc/ehvi.hip)
    def eval_posterior(self, hyps, want_report=False):
        """The posterior half of eval_nominate, kept (b7_eval_posterior): mean and variance of every hyper sample over the resident
        grid stay on the device for ehvi_nominate / posterior_get; no score, no arg-max, no accumulator afterwards.  A change of
        the grid or the data forgets it.  Returns None, or the report dict(jitter, info)."""
        S = len(hyps)
        arr, keep = self._pack_hyps(hyps, getattr(self, "_data_d", -1))
        jit = np.zeros(max(S, 1), dtype=np.float64) if want_report else None
        info = np.zeros(max(S, 1), dtype=np.int32) if want_report else None
        self._ck(self._L.b7_eval_posterior(self._h, S, arr, _ptr(jit), _ptr(info)))
        self.fit_token += 1
        return {"jitter": jit[:S], "info": info[:S]} if want_report else None

    def posterior_get(self, s):
        """(mean, var), one entry per grid row, of sample s (0-based) of the kept posterior (b7_posterior_get)."""
        M, _ = self.grid_shape()
        mean, var = np.empty(M, dtype=np.float64), np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_posterior_get(self._h, int(s), _ptr(mean), _ptr(var)))
        return mean, var

    def ehvi_compute(self, mu1, var1, mu2, var2, front, ref, _who="ehvi_compute"):
        """The marginal expected hypervolume improvement on host arrays by the nomination's own kernel (b7_ehvi_compute): mu1 / var1
        S1 x M of objective 1, mu2 / var2 S2 x M of objective 2, front P x 2 canonical (pareto_front2), ref (r1, r2) -> M scores."""
        mu1, var1, mu2, var2 = (np.atleast_2d(_f64(a)) for a in (mu1, var1, mu2, var2))
        front, ref = _f64(front).reshape(-1, 2), _f64(ref).ravel()
        M = mu1.shape[1]
        if var1.shape != mu1.shape or var2.shape != mu2.shape or mu2.shape[1] != M or ref.size != 2:
            raise Bot7HipError(-1, _who + ": mu1 / var1 S1 x M, mu2 / var2 S2 x M, front P x 2, ref 2")
        out = np.empty(M, dtype=np.float64)
        self._ck(getattr(self._L, "b7_" + _who)(self._h, _ptr(mu1), _ptr(var1), mu1.shape[0], _ptr(mu2), _ptr(var2), mu2.shape[0],
                                         _ptr(front), front.shape[0], _ptr(ref), M, _ptr(out)))
        return out

    def ehvi_nominate(self, other, front, ref, _who="ehvi_nominate"):
        """The two-objective nomination (b7_ehvi_nominate): this context holds objective 1's kept posterior (eval_posterior), `other`
        objective 2's (other may be this context).  Both must hold the same grid rows: the caller's contract, only the row count is
        checked.  The marginal score stays in this context's accumulator (score_finish(1, download=True) reads it).  Returns (value,
        1-based index); neither grid is modified."""
        if not isinstance(other, Context) or other._L is not self._L:
            raise Bot7HipError(-1, _who + ": other must be a Context of the same library")
        front, ref = _f64(front).reshape(-1, 2), _f64(ref).ravel()
        if ref.size != 2:
            raise Bot7HipError(-1, _who + ": ref has two entries")
        val, idx = C.c_double(), C.c_int64()
        self._ck(getattr(self._L, "b7_" + _who)(self._h, other._h, _ptr(front), front.shape[0], _ptr(ref), C.byref(val), C.byref(idx)))
        return val.value, idx.value

    # ---- three objectives: the expected hypervolume improvement over a box decomposition (csrc/ehvi3.hip)
    def ehvi3_compute(self, mu, var, front, ref, _who="ehvi3_compute"):
        """The marginal three-objective expected hypervolume improvement on host arrays by the nomination's own kernels
        (b7_ehvi3_compute): mu / var three arrays each, S_m x M of objective m, front P x 3 canonical (pareto_front3), ref
        (r1, r2, r3) -> M scores."""
        if len(mu) != 3 or len(var) != 3:
            raise Bot7HipError(-1, _who + ": mu and var hold one array per objective, three each")
        mu, var = [np.atleast_2d(_f64(a)) for a in mu], [np.atleast_2d(_f64(a)) for a in var]
        front, ref = _f64(front).reshape(-1, 3), _f64(ref).ravel()
        M = mu[0].shape[1]
        if any(v.shape != m.shape or m.shape[1] != M for m, v in zip(mu, var)) or ref.size != 3:
            raise Bot7HipError(-1, _who + ": mu[m] / var[m] S_m x M, front P x 3, ref 3")
        pm = (C.c_void_p * 3)(*[a.ctypes.data for a in mu])
        pv = (C.c_void_p * 3)(*[a.ctypes.data for a in var])
        S = (C.c_int * 3)(*[a.shape[0] for a in mu])
        out = np.empty(M, dtype=np.float64)
        self._ck(getattr(self._L, "b7_" + _who)(self._h, pm, pv, S, _ptr(front), front.shape[0], _ptr(ref), M, _ptr(out)))
        return out

    def ehvi3_nominate(self, other2, other3, front, ref, _who="ehvi3_nominate"):
        """The three-objective nomination (b7_ehvi3_nominate): this context holds objective 1's kept posterior (eval_posterior),
        other2 / other3 those of objectives 2 and 3 (contexts may coincide).  All must hold the same grid rows: the caller's
        contract, only the row count is checked.  The marginal score stays in this context's accumulator (score_finish(1,
        download=True) reads it).  Returns (value, 1-based index); no grid is modified."""
        for o in (other2, other3):
            if not isinstance(o, Context) or o._L is not self._L:
                raise Bot7HipError(-1, _who + ": other2 and other3 must be Contexts of the same library")
        front, ref = _f64(front).reshape(-1, 3), _f64(ref).ravel()
        if ref.size != 3:
            raise Bot7HipError(-1, _who + ": ref has three entries")
        val, idx = C.c_double(), C.c_int64()
        self._ck(getattr(self._L, "b7_" + _who)(self._h, other2._h, other3._h, _ptr(front), front.shape[0], _ptr(ref), C.byref(val), C.byref(idx)))
        return val.value, idx.value

    # ---- log-space EHVI (csrc/ehvi_math.h's EhviLog): the four calls above, in log space
    def logehvi_compute(self, mu1, var1, mu2, var2, front, ref):
        """log of ehvi_compute's marginal, evaluated so that it never underflows (b7_logehvi_compute); -inf is a legal value."""
        return self.ehvi_compute(mu1, var1, mu2, var2, front, ref, _who="logehvi_compute")

    def logehvi_nominate(self, other, front, ref):
        """ehvi_nominate by the log score (b7_logehvi_nominate): it still ranks the rows whose linear score is 0.  The marginal log
        score stays in this context's accumulator as a LOG accumulator: score_finish(1, download=True) reads it, and
        feas_add_acc(self) takes it (constrained multi-objective nomination: feas_reset, feas_add / feas_add_acc, feas_nominate)."""
        return self.ehvi_nominate(other, front, ref, _who="logehvi_nominate")

    def logehvi3_compute(self, mu, var, front, ref):
        """log of ehvi3_compute's marginal (b7_logehvi3_compute)."""
        return self.ehvi3_compute(mu, var, front, ref, _who="logehvi3_compute")

    def logehvi3_nominate(self, other2, other3, front, ref):
        """ehvi3_nominate by the log score (b7_logehvi3_nominate); the accumulator is a log one, as logehvi_nominate leaves it."""
        return self.ehvi3_nominate(other2, other3, front, ref, _who="logehvi3_nominate")

    def rff_compute(self, X, omega, phase, W):
        """cos(X omega' + phase) W on host arrays (b7_rff_compute): X M1 x d, omega F x d, phase F, W F x q -> M1 x q."""
        X, omega, phase, W = _f64(X), _f64(omega), _f64(phase).ravel(), _f64(W)
        if W.ndim == 1:
            W = W.reshape(-1, 1)
        if X.ndim != 2 or omega.ndim != 2 or omega.shape[1] != X.shape[1] or phase.size != omega.shape[0] or W.shape[0] != omega.shape[0]:
            raise Bot7HipError(-1, "rff_compute: X M1 x d, omega F x d, phase F, W F x q")
        out = np.empty((X.shape[0], W.shape[1]), dtype=np.float64)
        self._ck(self._L.b7_rff_compute(self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(omega), _ptr(phase), _ptr(W), omega.shape[0],
                                        W.shape[1], _ptr(out)))
        return out

    def ei_compute(self, mean, var, fmin, tradeoff=0.0):
        mean = _f64(mean)
        M = mean.shape[0]
        c = 1 if mean.ndim == 1 else mean.shape[1]
        var, fmin = _f64(var).ravel(), _f64(fmin).ravel()
        out = np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_ei_compute(self._h, _ptr(mean), _ptr(var), _ptr(fmin), float(tradeoff), M, c, _ptr(out)))
        return out

    def logei_compute(self, mean, var, fmin, tradeoff=0.0):
        """log EI on caller-provided mean (M or M x c) / var (M); c > 1: the log of the row mean of EI (b7_logei_compute)."""
        mean = _f64(mean)
        M = mean.shape[0]
        c = 1 if mean.ndim == 1 else mean.shape[1]
        var, fmin = _f64(var).ravel(), _f64(fmin).ravel()
        out = np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_logei_compute(self._h, _ptr(mean), _ptr(var), _ptr(fmin), float(tradeoff), M, c, _ptr(out)))
        return out

    def logpi_compute(self, mean, var, fmin, tradeoff=0.0):
        """log Phi(z) on caller-provided mean (M or M x c) / var (M); c > 1: the log of the row mean of Phi (b7_logpi_compute)."""
        mean = _f64(mean)
        M = mean.shape[0]
        c = 1 if mean.ndim == 1 else mean.shape[1]
        var, fmin = _f64(var).ravel(), _f64(fmin).ravel()
        out = np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_logpi_compute(self._h, _ptr(mean), _ptr(var), _ptr(fmin), float(tradeoff), M, c, _ptr(out)))
        return out

    def cb_compute(self, mean, var, tradeoff=1.0, upper=False, sign=-1.0):
        mean = _f64(mean)
        M = mean.shape[0]
        c = 1 if mean.ndim == 1 else mean.shape[1]
        var = _f64(var).ravel()
        out = np.empty(M, dtype=np.float64)
        self._ck(self._L.b7_cb_compute(self._h, _ptr(mean), _ptr(var), float(tradeoff), int(bool(upper)), float(sign),
                                       M, c, _ptr(out)))
        return out

    def argmax(self, scores):
        s = _f64(scores).ravel()
        v, i = C.c_double(), C.c_int64()
        self._ck(self._L.b7_argmax(self._h, _ptr(s), s.shape[0], C.byref(v), C.byref(i)))
        return v.value, i.value

    # ---- measurement
    def timer_start(self, slot=0):
        self._ck(self._L.b7_timer_start(self._h, slot))

    def timer_stop(self, slot=0):
        self._ck(self._L.b7_timer_stop(self._h, slot))

    def timer_ms(self, slot=0):
        ms = C.c_float()
        self._ck(self._L.b7_timer_ms(self._h, slot, C.byref(ms)))
        return ms.value

    def profile_enable(self, on=True):
        self._ck(self._L.b7_profile_enable(self._h, int(bool(on))))

    def profile_reset(self):
        self._ck(self._L.b7_profile_reset(self._h))

    def profile_get(self, phase):
        ms, n = C.c_double(), C.c_int64()
        self._ck(self._L.b7_profile_get(self._h, phase.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


class Group(object):
    """One host process, several GPUs (b7_group_*): a candidate grid sharded over the members, the observations on every
    member, bayesopt:eval + nominate over the union as one call.  device_ids may repeat (virtual ranks on one device)."""

    def __init__(self, device_ids, lib=None):
        self._L = load(lib)
        ids = np.ascontiguousarray(np.asarray(device_ids, dtype=np.int32).ravel())
        h = C.c_void_p()
        rc = self._L.b7_group_create(C.byref(h), ids.size, _ptr(ids))
        if rc != B7_OK:
            raise Bot7HipError(rc, (self._L.b7_last_error(None) or b"").decode())
        self._h, self.n = h, int(ids.size)
        self.members = [Context(int(ids[r]), _borrowed=self._L.b7_group_ctx(h, r), lib=lib) for r in range(self.n)]
        self._data_d = -1
        self.grid_version = 0

    def close(self):
        if getattr(self, "_h", None):
            for m in self.members:
                m.close()
            self._L.b7_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != B7_OK:
            raise Bot7HipError(rc, (self._L.b7_group_last_error(self._h) or b"").decode())

    def info(self):
        n, r = C.c_int(), C.c_int()
        self._ck(self._L.b7_group_info(self._h, C.byref(n), C.byref(r)))
        return {"n": n.value, "uses_rccl": bool(r.value)}

    def set_workspace(self, nbytes):
        self._ck(self._L.b7_group_set_workspace(self._h, int(nbytes)))

    def gp_set_kernel(self, kernel):
        """b7_gp_set_kernel on every member (Context.gp_set_kernel)."""
        code = kernel_code(kernel)
        if any(m.kernel != code for m in self.members):
            self._ck(self._L.b7_group_gp_set_kernel(self._h, code))
            for m in self.members:
                if m.kernel != code:
                    m.kernel = code
                    m.fit_token += 1

    def grid_sobol(self, size, dims, skip=1, mins=None, maxes=None):
        mn, mx = Context._minmax(mins, maxes, dims)
        self._ck(self._L.b7_group_grid_sobol(self._h, int(size), int(dims), int(skip), _ptr(mn), _ptr(mx)))
        self.grid_version += 1

    def grid_random(self, size, dims, seed=0, mins=None, maxes=None):
        mn, mx = Context._minmax(mins, maxes, dims)
        self._ck(self._L.b7_group_grid_random(self._h, int(size), int(dims), int(seed) & (2 ** 64 - 1), _ptr(mn), _ptr(mx)))
        self.grid_version += 1

    def grid_upload(self, X):
        X = _f64(X)
        self._ck(self._L.b7_group_grid_upload(self._h, _ptr(X), X.shape[0], X.shape[1]))
        self.grid_version += 1

    def grid_shape(self):
        M, d, off = C.c_int64(), C.c_int(), np.zeros(self.n + 1, dtype=np.int64)
        self._ck(self._L.b7_group_grid_shape(self._h, C.byref(M), C.byref(d), _ptr(off)))
        return M.value, d.value, off

    def grid_download(self, row0=0, rows=None):
        M, d, _ = self.grid_shape()
        rows = M - row0 if rows is None else rows
        out = np.empty((rows, d), dtype=np.float64)
        self._ck(self._L.b7_group_grid_download(self._h, int(row0), int(rows), _ptr(out)))
        return out

    def grid_remove_rows(self, idx1, want_rows=True):
        idx = np.ascontiguousarray(np.asarray(idx1, dtype=np.int64).ravel())
        _, d, _ = self.grid_shape()
        rows = np.empty((idx.size, d), dtype=np.float64) if want_rows else None
        self._ck(self._L.b7_group_grid_remove_rows(self._h, _ptr(idx), idx.size, _ptr(rows)))
        self.grid_version += 1
        return rows

    def gp_set_data(self, X_obs, Y_obs):
        X = _f64(X_obs)
        Y = _f64(Y_obs)
        if Y.ndim == 1:
            Y = Y.reshape(-1, 1)
        self._ck(self._L.b7_group_gp_set_data(self._h, _ptr(X), _ptr(Y), X.shape[0], X.shape[1], Y.shape[1]))
        self._data_d = X.shape[1]
        for m in self.members:
            m._data_d = X.shape[1]
            m.ycols = Y.shape[1]
            m.fit_token += 1

    def eval_nominate(self, hyps, score="ei", fmin=None, tradeoff=None, upper=False, sign=-1.0, want_report=False, levels=None):
        if levels is not None:   # as Context.eval_nominate: the members' level count (the group call itself refuses score "mes")
            for m in self.members:
                m.mes_set_levels(levels)
        S = len(hyps)
        arr, keep = Context._pack_hyps(hyps, self._data_d)
        spec, fm = Context._pack_spec(score, fmin, tradeoff, upper, sign)
        jit = np.zeros(S, dtype=np.float64) if want_report else None
        info = np.zeros(S, dtype=np.int32) if want_report else None
        v, i = C.c_double(), C.c_int64()
        self._ck(self._L.b7_group_eval_nominate(self._h, S, arr, C.byref(spec), C.byref(v), C.byref(i), _ptr(jit), _ptr(info)))
        if want_report:
            return v.value, i.value, {"jitter": jit, "info": info}
        return v.value, i.value

    def nominate_commit(self, idx1_global):
        _, d, _ = self.grid_shape()
        row = np.empty(d, dtype=np.float64)
        self._ck(self._L.b7_group_nominate_commit(self._h, int(idx1_global), _ptr(row)))
        self.grid_version += 1
        return row


def torch_rand(seed, n, resolution=32):
    """torch.manualSeed(seed); torch.rand(n) -- MT19937, host-only."""
    out = np.empty(int(n), dtype=np.float64)
    rc = load().b7_torch_rand(int(seed), int(n), int(resolution), _ptr(out))
    if rc != B7_OK:
        raise Bot7HipError(rc, "resolution must be 32 or 53")
    return out


def shard_commit_rule(idx1_global, offset, M_local):
    """The library's bookkeeping rule for a stable deletion on the union of contiguous shards -> (local_idx1, new_offset).
    Host-only."""
    loc, off = C.c_int64(), C.c_int64()
    rc = load().b7_shard_commit_rule(int(idx1_global), int(offset), int(M_local), C.byref(loc), C.byref(off))
    if rc != B7_OK:
        raise Bot7HipError(rc, "bad index / offset")
    return loc.value, off.value


COMM_ID_BYTES = 128


def comm_unique_id():
    """ncclGetUniqueId through the C ABI (rank 0 calls it and distributes the 128 bytes)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().b7_comm_unique_id(C.cast(buf, C.c_void_p))
    if rc != B7_OK:
        raise Bot7HipError(rc, (load().b7_last_error(None) or b"").decode())
    return buf.raw


def comm_pick_winner(pairs):
    """The library's winner rule on a list of (value, global_idx1) pairs (idx1 <= 0: empty shard).  Host-only."""
    tab = np.zeros((len(pairs), 2), dtype=np.uint64)
    for r, (v, i) in enumerate(pairs):
        if int(i) > 0:
            tab[r, 0] = np.array([v], dtype=np.float64).view(np.uint64)[0]
            tab[r, 1] = int(i)
    v, i = C.c_double(), C.c_int64()
    rc = load().b7_comm_pick_winner(_ptr(tab), len(pairs), C.byref(v), C.byref(i))
    if rc != B7_OK:
        raise Bot7HipError(rc, "every shard is empty")
    return v.value, i.value


def tr_box(hyps, center, length, mins, maxes):
    """The trust region's box (lo, hi) around `center` from the hyper samples' ARD lengthscales: hyps as eval_nominate takes them
    (dicts or (lenscale_sq, amp, noise, mean)), or bare lenscale_sq vectors -- only the lengthscales are read.  Host-only (b7_tr_box)."""
    center, mins, maxes = _f64(center).ravel(), _f64(mins).ravel(), _f64(maxes).ravel()
    d = center.size
    if mins.size != d or maxes.size != d:
        raise Bot7HipError(-1, "tr_box: center, mins and maxes have the same number of entries")
    arr, keep = Context._pack_hyps([h if isinstance(h, (dict, tuple)) else (h, 1.0, 0.0, 0.0) for h in hyps], d)
    lo, hi = np.empty(d), np.empty(d)
    rc = load().b7_tr_box(d, len(keep), arr, _ptr(center), float(length), _ptr(mins), _ptr(maxes), _ptr(lo), _ptr(hi))
    if rc != B7_OK:
        raise Bot7HipError(rc, "tr_box: S >= 1, lenscale_sq > 0, maxes > mins, length > 0, all finite, and the center inside [mins, maxes]")
    return lo, hi


class TrustRegionState(object):
    """The trust region's side length and the success / failure counters that resize it (b7_tr_state, b7_tr_init, b7_tr_update).
    A parameter <= 0 (or None) takes the library's default."""

    FIELDS = ("length", "length_init", "length_min", "length_max", "best", "succ", "fail", "succ_tol", "fail_tol", "restarts")

    def __init__(self, d, q=1, length_init=None, length_min=None, length_max=None, succ_tol=None, fail_tol=None):
        self._st, self.q = TrState(), int(q)
        rc = load().b7_tr_init(C.byref(self._st), int(d), int(q), float(length_init or 0.0), float(length_min or 0.0),
                               float(length_max or 0.0), int(succ_tol or 0), int(fail_tol or 0))
        if rc != B7_OK:
            raise Bot7HipError(rc, "tr_init: d >= 1, q >= 1, finite lengths with length_min <= length_init <= length_max")

    def __getattr__(self, name):
        if name in TrustRegionState.FIELDS:
            return getattr(self._st, name)
        raise AttributeError(name)

    def update(self, y):
        """One trial's responses (minimised) -> True when the region collapsed and the state restarted."""
        y = _f64(y).ravel()
        restart = C.c_int(0)
        rc = load().b7_tr_update(C.byref(self._st), _ptr(y), y.size, C.byref(restart))
        if rc != B7_OK:
            raise Bot7HipError(rc, "tr_update: at least one response")
        return bool(restart.value)

    def as_dict(self):
        return {k: getattr(self._st, k) for k in TrustRegionState.FIELDS}


def pareto_front2(Y, ref):
    """The canonical front of n rows of two responses (minimised) under the reference point ref = (r1, r2): rows with a non-finite
    entry or not strictly inside the box dropped, dominated rows dropped, of equal rows the lowest kept, sorted with the first
    objective ascending.  Returns (front P x 2, rows P: each point's 1-based source row).  Host-only (b7_pareto_front2); more than
    EHVI_PMAX points raise."""
    Y, ref = _f64(Y).reshape(-1, 2), _f64(ref).ravel()
    if ref.size != 2:
        raise Bot7HipError(-1, "pareto_front2: ref has two entries")
    cap = max(1, min(Y.shape[0], EHVI_PMAX))
    front, rows, P = np.empty((cap, 2), dtype=np.float64), np.zeros(cap, dtype=np.int64), C.c_int()
    rc = load().b7_pareto_front2(_ptr(Y), Y.shape[0], _ptr(ref), _ptr(front), _ptr(rows), C.byref(P))
    if rc != B7_OK:
        raise Bot7HipError(rc, "pareto_front2: a front of %d points (at most %d are built)" % (P.value, EHVI_PMAX) if P.value > EHVI_PMAX
                           else "pareto_front2: the reference point must be finite")
    return front[:P.value].copy(), rows[:P.value].copy()


def hypervolume2(front, ref):
    """The area a canonical front (pareto_front2) dominates inside the reference box.  Host-only (b7_hypervolume2)."""
    front, ref = _f64(front).reshape(-1, 2), _f64(ref).ravel()
    if ref.size != 2:
        raise Bot7HipError(-1, "hypervolume2: ref has two entries")
    hv = C.c_double()
    rc = load().b7_hypervolume2(_ptr(front), front.shape[0], _ptr(ref), C.byref(hv))
    if rc != B7_OK:
        raise Bot7HipError(rc, "hypervolume2: the front is not canonical (strictly inside a finite reference box, the first objective "
                               "strictly ascending, the second strictly descending)")
    return hv.value


def pareto_front3(Y, ref):
    """The canonical front of n rows of three responses (minimised) under the reference point ref = (r1, r2, r3): rows with a
    non-finite entry or not strictly inside the box dropped, dominated rows dropped, of equal rows the lowest kept, sorted by (third,
    first, second) objective.  Returns (front P x 3, rows P: each point's 1-based source row).  Host-only (b7_pareto_front3); more
    than EHVI3_PMAX points raise."""
    Y, ref = _f64(Y).reshape(-1, 3), _f64(ref).ravel()
    if ref.size != 3:
        raise Bot7HipError(-1, "pareto_front3: ref has three entries")
    cap = max(1, min(Y.shape[0], EHVI3_PMAX))
    front, rows, P = np.empty((cap, 3), dtype=np.float64), np.zeros(cap, dtype=np.int64), C.c_int()
    rc = load().b7_pareto_front3(_ptr(Y), Y.shape[0], _ptr(ref), _ptr(front), _ptr(rows), C.byref(P))
    if rc != B7_OK:
        raise Bot7HipError(rc, "pareto_front3: a front of %d points (at most %d are built)" % (P.value, EHVI3_PMAX) if P.value > EHVI3_PMAX
                           else "pareto_front3: the reference point must be finite")
    return front[:P.value].copy(), rows[:P.value].copy()


_CANONICAL3 = ("the front is not canonical (strictly inside a finite reference box, mutually non-dominated, strictly ascending by the "
               "third, then the first, then the second objective, at most %d points)" % EHVI3_PMAX)


def nondominated_boxes3(front, ref):
    """The region no point of a canonical front (pareto_front3) dominates, inside (-inf, ref], as disjoint boxes B x 5: l1, u1, l2, u2,
    u3 (the lower edge in the third objective is -inf; -inf is a legal l1 / l2).  Host-only (b7_nondominated_boxes3)."""
    front, ref = _f64(front).reshape(-1, 3), _f64(ref).ravel()
    if ref.size != 3:
        raise Bot7HipError(-1, "nondominated_boxes3: ref has three entries")
    boxes, B = np.empty((3 * front.shape[0] + 1, 5), dtype=np.float64), C.c_int()
    rc = load().b7_nondominated_boxes3(_ptr(front), front.shape[0], _ptr(ref), _ptr(boxes), C.byref(B))
    if rc != B7_OK:
        raise Bot7HipError(rc, "nondominated_boxes3: " + _CANONICAL3)
    return boxes[:B.value].copy()


def hypervolume3(front, ref):
    """The volume a canonical front (pareto_front3) dominates inside the reference box.  Host-only (b7_hypervolume3)."""
    front, ref = _f64(front).reshape(-1, 3), _f64(ref).ravel()
    if ref.size != 3:
        raise Bot7HipError(-1, "hypervolume3: ref has three entries")
    hv = C.c_double()
    rc = load().b7_hypervolume3(_ptr(front), front.shape[0], _ptr(ref), C.byref(hv))
    if rc != B7_OK:
        raise Bot7HipError(rc, "hypervolume3: " + _CANONICAL3)
    return hv.value


def sobol_direction_numbers(dims):
    """Host-only view of the Sobol direction-number table the kernel uses (no GPU needed)."""
    out = np.empty((dims, 30), dtype=np.uint32)
    rc = load().b7_sobol_direction_numbers(int(dims), _ptr(out))
    if rc != B7_OK:
        raise Bot7HipError(rc, "dims must be in [1, 39]")
    return out


_default = {}


def default_context(device_id=None):
    """Process-wide context for a device (LOCAL_RANK when launched one process per GPU)."""
    if device_id is None:
        device_id = int(os.environ.get("LOCAL_RANK", "0"))
    if device_id not in _default:
        _default[device_id] = Context(device_id)
    return _default[device_id]
