"""ctypes binding of libaa_hip.so (include/aa_hip.h) -- the only way this package
computes.  There is NO CPU fallback: if the library is missing, or no MI355X is
visible, every numeric entry point raises ``RuntimeError``.

Host code is plain NumPy (the reference package is NumPy-only); device memory is
owned by an ``aa_ctx`` created and destroyed inside each estimator call, so estimator
instances hold no device handles and stay ``copy.deepcopy``-safe (the drivers deepcopy
models: bin/run_hadisst_aa.py:171).
"""
import atexit
import ctypes
import os
import threading
import zlib

import numpy as np

AA_F32, AA_F64 = 0, 1
FORM_DATA, FORM_KERNEL = 0, 1
MAX_K = 64
GRAM_SIDES = ("rows", "cols")    # AA_GRAM_ROWS, AA_GRAM_COLS
GRAM_MAX_D = 8192                # largest Gram matrix aa_data_gram forms (it goes through one host eigen-solve)
MAX_PROJECTED = 256              # AA_MAX_PROJECTED: most directions of aa_set_data_projected
MAX_SLOTS = 1464                 # AA_MAX_SLOTS: most calendar slots of aa_data_slot_sums / aa_set_data_rows_slots
SLOT_CHUNK_ROWS = 64             # AA_SLOT_CHUNK_ROWS: most rows of one slot a work item of the slot kernels walks
SLOT_TILE_COLS = 256             # AA_SLOT_TILE_COLS: adjacent columns of a work item
DIAG_KINDS = ("given", "ones", "poly", "linear")     # AA_DIAG_*: where aa_kernel_sample_residuals takes kappa(y, y) from

SPG_FLAG_CONVERGED = 1
SPG_FLAG_LAMBDA_MIN = 2
SPG_FLAG_MAX_FEVAL = 4
SPG_FLAG_MAX_ITER = 8
SPG_FLAG_PROJ_UNCONV = 16

_LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                         "libaa_hip.so")

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


class QPParams(ctypes.Structure):
    """aa_qp_params: keyword arguments of quad_simplex_spg (reference spg.py:287-291)."""
    _fields_ = [("gamma", ctypes.c_double), ("memory", ctypes.c_int),
                ("sigma_one", ctypes.c_double), ("sigma_two", ctypes.c_double),
                ("lambda_min", ctypes.c_double), ("alpha0", ctypes.c_double),
                ("alpha_min", ctypes.c_double), ("alpha_max", ctypes.c_double),
                ("epsilon_one", ctypes.c_double), ("epsilon_two", ctypes.c_double),
                ("max_iterations", ctypes.c_int), ("max_feval", ctypes.c_int)]


class SPGParams(ctypes.Structure):
    """aa_spg_params: keyword arguments of spg (reference spg.py:46-51)."""
    _fields_ = [("gamma", ctypes.c_double), ("memory", ctypes.c_int),
                ("sigma_one", ctypes.c_double), ("sigma_two", ctypes.c_double),
                ("lambda_min", ctypes.c_double), ("alpha0", ctypes.c_double),
                ("alpha_min", ctypes.c_double), ("alpha_max", ctypes.c_double),
                ("epsilon_one", ctypes.c_double), ("epsilon_two", ctypes.c_double),
                ("use_infinity_norm", ctypes.c_int),
                ("max_iterations", ctypes.c_int), ("max_feval", ctypes.c_int)]


class SPGStats(ctypes.Structure):
    _fields_ = [("f", ctypes.c_double), ("n_iter", ctypes.c_int), ("n_feval", ctypes.c_int),
                ("flags", ctypes.c_int), ("res_norm", ctypes.c_double)]


class IterParams(ctypes.Structure):
    """aa_iter_params: the loop controls of _iterate_aa (reference archetypal_analysis.py:534-541)."""
    _fields_ = [("max_outer", ctypes.c_int), ("tolerance", ctypes.c_double),
                ("criterion", ctypes.c_int), ("require_monotonic", ctypes.c_int),
                ("mono_tolerance", ctypes.c_double),
                ("update_dictionary", ctypes.c_int), ("update_weights", ctypes.c_int),
                ("check_every", ctypes.c_int), ("delta", ctypes.c_double)]


class IterStats(ctypes.Structure):
    _fields_ = [("n_iter", ctypes.c_int), ("converged", ctypes.c_int),
                ("error_stage", ctypes.c_int), ("error_iter", ctypes.c_int),
                ("spg_flags", ctypes.c_int), ("reserved", ctypes.c_int), ("cost", ctypes.c_double)]


class GPNHParams(ctypes.Structure):
    """aa_gpnh_params: lambda_W plus the loop controls."""
    _fields_ = [("lambda_W", ctypes.c_double), ("loop", IterParams)]


class SlotStatus(ctypes.Structure):
    """aa_slot_status: one restart slot of aa_gpnh_slots_run / aa_slots_run.  ``flags``: GPNH -- nonzero when
    the slot's normal equations were not positive definite; AA -- the slot's SPG_FLAG_* warning bits."""
    _fields_ = [("stop", ctypes.c_int), ("converged", ctypes.c_int), ("error_stage", ctypes.c_int),
                ("stop_iter", ctypes.c_int), ("flags", ctypes.c_int), ("iterations_run", ctypes.c_int)]


class QPStats(ctypes.Structure):
    _fields_ = [("total_passes", ctypes.c_long), ("max_passes", ctypes.c_int),
                ("reserved", ctypes.c_int)]


# name -> (restype, argtypes); every symbol include/aa_hip.h declares
_vp = ctypes.c_void_p
_SIGNATURES = {
    "aa_last_error": (ctypes.c_char_p, []),
    "aa_version": (ctypes.c_int, []),
    "aa_device_count": (ctypes.c_int, [_ip]),
    "aa_set_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "aa_simplex_project_rows": (ctypes.c_int, [ctypes.c_int, _dp, _dp, ctypes.c_long, ctypes.c_long]),
    "aa_quad_simplex_spg_batch": (ctypes.c_int, [ctypes.c_int, _dp, _dp, ctypes.c_long, ctypes.c_long,
                                                 _dp, _dp, ctypes.c_long, ctypes.c_int,
                                                 ctypes.POINTER(QPParams), _ip]),
    "aa_ctx_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int]),
    "aa_ctx_destroy": (ctypes.c_int, [_vp]),
    "aa_comm_get_unique_id": (ctypes.c_int, [_vp]),
    "aa_ctx_comm_init": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int]),
    "aa_ctx_p2p_export": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "aa_ctx_p2p_init": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int]),
    "aa_ctx_allreduce_host": (ctypes.c_int, [_vp, _dp, ctypes.c_int, ctypes.c_int]),
    "aa_set_data": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                   ctypes.c_int, ctypes.c_long, ctypes.c_long]),
    "aa_data_trace": (ctypes.c_int, [_vp, _dp]),
    "aa_set_linear_kernel": (ctypes.c_int, [_vp, ctypes.c_int]),
    "aa_set_rbf_features": (ctypes.c_int, [_vp, _dp, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_double]),
    "aa_set_poly_features": (ctypes.c_int, [_vp, _dp, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_int]),
    "aa_set_rbf_features_resident": (ctypes.c_int, [_vp, _vp, ctypes.c_double]),
    "aa_set_poly_features_resident": (ctypes.c_int, [_vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int]),
    "aa_set_data_take": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_long), ctypes.c_long]),
    "aa_kernel_sample_residuals": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp]),
    "aa_share_data": (ctypes.c_int, [_vp, _vp]),
    "aa_set_data_rows": (ctypes.c_int, [_vp, _vp, ctypes.c_long, ctypes.c_long]),
    "aa_set_data_rows_affine": (ctypes.c_int, [_vp, _vp, ctypes.c_long, ctypes.c_long, _dp, _dp]),
    "aa_data_column_moments": (ctypes.c_int, [_vp, _dp, _dp]),
    "aa_data_weighted_column_sums": (ctypes.c_int, [_vp, ctypes.c_int, _dp, _dp]),
    "aa_data_grouped_sqdev": (ctypes.c_int, [_vp, ctypes.c_int, _dp, _ip, _dp, ctypes.c_int, _dp]),
    "aa_set_data_rows_model": (ctypes.c_int, [_vp, _vp, ctypes.c_long, ctypes.c_long, ctypes.c_int, _ip, _dp, _dp, _dp,
                                              _dp, _dp]),
    "aa_data_slot_sums": (ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _dp, ctypes.POINTER(ctypes.c_long)]),
    "aa_set_data_rows_slots": (ctypes.c_int, [_vp, _vp, ctypes.c_long, ctypes.c_long, ctypes.c_int, _ip, _dp, _dp]),
    "aa_data_gram": (ctypes.c_int, [_vp, ctypes.c_int, _dp, _dp, ctypes.c_long]),
    "aa_set_data_projected": (ctypes.c_int, [_vp, _vp, ctypes.c_long, ctypes.c_long, ctypes.c_int, _dp, ctypes.c_long,
                                             _dp]),
    "aa_set_data_weighted": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                            _dp, ctypes.c_long, ctypes.c_long,
                                            ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_long)]),
    "aa_get_data": (ctypes.c_int, [_vp, _dp, ctypes.c_long]),
    "aa_set_state": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, _dp, _dp]),
    "aa_get_state": (ctypes.c_int, [_vp, _dp, ctypes.c_long, _dp, _dp]),
    "aa_set_alpha": (ctypes.c_int, [_vp, _dp]),
    "aa_prepare": (ctypes.c_int, [_vp, _dp]),
    "aa_cost": (ctypes.c_int, [_vp, _dp]),
    "aa_get_grams": (ctypes.c_int, [_vp, _dp, _dp, _dp, _dp]),
    "aa_set_dictionary_inputs": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_double]),
    "aa_dictionary_update": (ctypes.c_int, [_vp, ctypes.POINTER(SPGParams), ctypes.POINTER(SPGStats)]),
    "aa_weights_update": (ctypes.c_int, [_vp, ctypes.POINTER(QPParams), ctypes.POINTER(QPStats)]),
    "aa_outer_iterations": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(SPGParams),
                                           ctypes.POINTER(QPParams), _dp]),
    "aa_iterate": (ctypes.c_int, [_vp, ctypes.POINTER(IterParams), ctypes.POINTER(SPGParams),
                                  ctypes.POINTER(QPParams), ctypes.POINTER(SPGParams), ctypes.c_double, _dp,
                                  ctypes.POINTER(IterStats)]),
    "aa_reconstruction_cost": (ctypes.c_int, [_vp, _dp]),
    "aa_get_archetypes": (ctypes.c_int, [_vp, _dp, ctypes.c_long]),
    "aa_distance_column": (ctypes.c_int, [_vp, ctypes.c_long, _dp]),
    "aa_furthest_sum": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_long, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                       ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "aa_get_furthest_sum_state": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_int), _dp,
                                                 ctypes.POINTER(ctypes.c_ubyte), _dp, ctypes.POINTER(ctypes.c_int),
                                                 ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "aa_gpnh_set_factors": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, _dp]),
    "aa_gpnh_get_weights": (ctypes.c_int, [_vp, _dp]),
    "aa_gpnh_reduce": (ctypes.c_int, [_vp, _dp, ctypes.c_long, _dp, _dp]),
    "aa_gpnh_weights_update": (ctypes.c_int, [_vp, _dp, ctypes.POINTER(QPParams), ctypes.POINTER(QPStats)]),
    "aa_gpnh_residual_cost": (ctypes.c_int, [_vp, _dp]),
    "aa_gpnh_residual_scores": (ctypes.c_int, [_vp, _dp, _dp, _dp]),
    "aa_set_rbf_reference": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, ctypes.c_long, ctypes.c_long, _dp,
                                            ctypes.c_long, ctypes.c_double]),
    "aa_rbf_cross": (ctypes.c_int, [_vp, _dp]),
    "aa_set_poly_reference": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, ctypes.c_long, ctypes.c_long, _dp,
                                             ctypes.c_long, ctypes.c_double, ctypes.c_double, ctypes.c_int]),
    "aa_poly_cross": (ctypes.c_int, [_vp, _dp]),
    "aa_kernel_transform_cost": (ctypes.c_int, [_vp, _dp, _dp, _dp]),
    "aa_gpnh_iterate": (ctypes.c_int, [_vp, ctypes.POINTER(GPNHParams), ctypes.POINTER(QPParams), _dp, _dp,
                                       ctypes.POINTER(IterStats)]),
    "aa_gpnh_get_dictionary": (ctypes.c_int, [_vp, _dp, ctypes.c_long]),
    "aa_gpnh_slots_begin": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GPNHParams),
                                           ctypes.POINTER(QPParams)]),
    "aa_gpnh_slots_load": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, _dp]),
    "aa_gpnh_slots_run": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(SlotStatus)]),
    "aa_gpnh_slots_fetch": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, _dp, _dp, _dp]),
    "aa_slots_begin": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(IterParams),
                                      ctypes.POINTER(SPGParams), ctypes.POINTER(QPParams), ctypes.POINTER(SPGParams)]),
    "aa_slots_load": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, _dp, _dp]),
    "aa_slots_run": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(SlotStatus)]),
    "aa_slots_reload": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, _dp, _dp]),
    "aa_slots_fetch": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, _dp, _dp, ctypes.c_long, ctypes.c_int,
                                      _dp, _dp, _dp]),
    "aa_slots_end": (ctypes.c_int, [_vp]),
    "aa_get_spg_scalars": (ctypes.c_int, [_vp, _dp]),
    "aa_pass_reduce_rows": (ctypes.c_int, [_vp, ctypes.c_int, _dp, _dp, ctypes.c_long]),
    "aa_pass_reduce_rows_flagged": (ctypes.c_int, [_vp, ctypes.c_int, _dp, _dp, ctypes.c_long]),
    "aa_reduce_sparse_counts": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_long)]),
    "aa_pass_row_local": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_long, _dp]),
    "aa_time_kernel": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _dp]),
    "aa_gemm_timing": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.POINTER(ctypes.c_int), _dp,
                                      ctypes.POINTER(ctypes.c_int)]),
    "aa_pass_kernels": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int]),
    "aa_proj_counts": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_long)]),
    "aa_qp_kernels": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    "aa_get_spg_array": (ctypes.c_int, [_vp, ctypes.c_int, _dp]),
    "aa_spg_path": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int]),
}

EXPORTED_SYMBOLS = tuple(sorted(_SIGNATURES))

_lib = None


def library_path():
    return _LIB_PATH


def load_library():
    """Load libaa_hip.so and bind every entry point.  Raises RuntimeError (never
    falls back) when the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            "convex_dim_red (MI355X build): %s not found -- build it with "
            "`python __graft_entry__.py` or `make -C matrix-factorization-case-studies_amd/csrc`. "
            "This package has no CPU fallback." % _LIB_PATH)
    lib = ctypes.CDLL(_LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    # tuning knobs from the environment: AA_HIP_OPTIONS="name=value,name=value" (aa_set_option)
    for item in filter(None, os.environ.get("AA_HIP_OPTIONS", "").split(",")):
        name, _, value = item.partition("=")
        if lib.aa_set_option(name.strip().encode(), int(value)) != 0:
            raise RuntimeError("AA_HIP_OPTIONS: bad option %r" % item)
    return lib


def _check(rc):
    if rc != 0:
        msg = load_library().aa_last_error()
        raise RuntimeError("libaa_hip error %d: %s" % (rc, msg.decode() if msg else "?"))


def distributed_env():
    """``(rank, local_rank, world)`` when this process is one rank of a one-process-per-GPU launch
    (``python -m torch.distributed.run --nproc-per-node N driver.py`` or any launcher that exports
    RANK / LOCAL_RANK / WORLD_SIZE) AND row sharding was asked for with
    ``CONVEX_DIM_RED_DISTRIBUTED=1``; ``None`` otherwise.  In that mode every rank runs the same
    driver (same data, same seeds): ``ArchetypalAnalysis`` / ``GPNHConvexCoding`` keep rows
    ``[n r / N, n (r + 1) / N)`` of the data matrix on their GPU, RCCL all-reduces the small Gram
    products (csrc/comm.hip), and every rank returns the full factors."""
    if os.environ.get("CONVEX_DIM_RED_DISTRIBUTED", "0") != "1":
        return None
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1 and os.environ.get("AA_FORCE_RCCL", "0") != "1":
        return None
    rank = int(os.environ.get("RANK", "0"))
    return rank, int(os.environ.get("LOCAL_RANK", str(rank))), world


def device_index():
    env = os.environ.get("CONVEX_DIM_RED_DEVICE")
    if env is not None:
        return int(env)
    dist = distributed_env()
    if dist is not None:
        return dist[1]
    return int(os.environ.get("LOCAL_RANK", "0")) if "CONVEX_DIM_RED_USE_LOCAL_RANK" in os.environ else 0


def default_dtype():
    v = os.environ.get("CONVEX_DIM_RED_DTYPE", "float64")
    if v not in ("float64", "float32"):
        raise ValueError("CONVEX_DIM_RED_DTYPE must be float64 or float32, got %r" % v)
    return v


def dtype_code(dtype):
    if dtype is None:
        dtype = default_dtype()
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return AA_F64
    if dtype == np.float32:
        return AA_F32
    raise ValueError("unsupported dtype %r (float64 or float32)" % (dtype,))


def check_component_count(k, whom, defaulted_from=None):
    """The device arrays hold 32 or 64 component slots: a model with more
    components is refused where its hyper-parameters are checked -- before any data moves -- and
    the message names the reference default that leads there."""
    if isinstance(k, (int, np.integer)) and k > MAX_K:
        hint = ""
        if defaulted_from is not None:
            hint = (" (n_components=None defaults to %s in the reference, archetypal_analysis.py:785-786 / "
                    "gpnh_convex_coding.py:508-509: pass n_components <= %d explicitly)" % (defaulted_from, MAX_K))
        raise ValueError("%s: n_components = %d exceeds the %d component slots of the MI355X build%s"
                         % (whom, k, MAX_K, hint))


def require_gpu():
    lib = load_library()
    n = ctypes.c_int(0)
    rc = lib.aa_device_count(ctypes.byref(n))
    if rc != 0 or n.value < 1:
        msg = lib.aa_last_error()
        raise RuntimeError("convex_dim_red (MI355X build): no HIP device available (%s); "
                           "this package has no CPU fallback"
                           % (msg.decode() if msg else "device count = %d" % n.value))
    return n.value


def set_option(name, value):
    """Process-wide tuning knob of the library (see include/aa_hip.h: aa_set_option)."""
    _check(load_library().aa_set_option(name.encode(), int(value)))


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def qp_params(**kw):
    """Defaults of _update_kernel_aa_weights (reference archetypal_analysis.py:372-383)."""
    return QPParams(kw.get("gamma", 1e-4), int(kw.get("memory", 1)),
                    kw.get("sigma_one", 0.1), kw.get("sigma_two", 0.9),
                    kw.get("lambda_min", 1e-10), kw.get("alpha0", -1.0),
                    kw.get("alpha_min", 1e-5), kw.get("alpha_max", 1e3),
                    kw.get("epsilon_one", 1e-10), kw.get("epsilon_two", 1e-6),
                    int(kw.get("max_iterations", 1000)), int(kw.get("max_feval", 2000)))


_SPG_KEYS = ("gamma", "memory", "sigma_one", "sigma_two", "lambda_min", "alpha0", "alpha_min",
             "alpha_max", "epsilon_one", "epsilon_two", "use_infinity_norm", "verbose",
             "max_iterations", "max_feval")


def _iter_params(max_outer, tolerance, stopping_criterion, require_monotonic, mono_tolerance, update_dictionary,
                 update_weights, check_every, delta):
    """aa_iter_params from the estimators' loop controls (``mono_tolerance`` None: the tolerance)."""
    crit = {"abs_delta_f": 0, "rel_delta_f": 1}.get(stopping_criterion)
    if crit is None:
        raise ValueError("unsupported stopping criterion '%s'" % stopping_criterion)
    return IterParams(int(max_outer), float(tolerance), crit, int(bool(require_monotonic)),
                      float(tolerance if mono_tolerance is None else mono_tolerance),
                      int(bool(update_dictionary)), int(bool(update_weights)), int(check_every), float(delta))


def spg_params(**kw):
    """Defaults of spg (reference spg.py:46-51); unknown keywords raise TypeError like the
    reference's call would."""
    for key in kw:
        if key not in _SPG_KEYS:
            raise TypeError("spg() got an unexpected keyword argument %r" % key)
    alpha0 = kw.get("alpha0", None)
    return SPGParams(kw.get("gamma", 1e-4), int(kw.get("memory", 1)),
                     kw.get("sigma_one", 0.1), kw.get("sigma_two", 0.9),
                     kw.get("lambda_min", 1e-10), -1.0 if alpha0 is None else float(alpha0),
                     kw.get("alpha_min", 1e-5), kw.get("alpha_max", 1e3),
                     kw.get("epsilon_one", 1e-10), kw.get("epsilon_two", 1e-6),
                     1 if kw.get("use_infinity_norm", True) else 0,
                     int(kw.get("max_iterations", 10000)), int(kw.get("max_feval", 1000000)))


# ---------------------------------------------------------------- stateless ops
def simplex_project_rows(A):
    require_gpu()
    A = _c64(A)
    if A.ndim != 2:
        raise ValueError("expected a 2-D array")
    out = np.empty_like(A)
    _check(load_library().aa_simplex_project_rows(device_index(), _ptr(A), _ptr(out),
                                                  A.shape[0], A.shape[1]))
    return out


def qp_batch(A, B, Z0, layout, return_iters=False, **kw):
    """layout 'kn': B is k x n, b_t = -B[:, t]; 'nk': B is n x k, b_t = -B[t]."""
    require_gpu()
    A, B, Z0 = _c64(A), _c64(B), _c64(Z0)
    n, k = Z0.shape
    if k > MAX_K:
        raise ValueError("n_components = %d exceeds the HIP backend limit of %d" % (k, MAX_K))
    sj, st = (n, 1) if layout == "kn" else (1, k)
    Z = np.empty_like(Z0)
    iters = np.zeros(n, dtype=np.int32)
    p = qp_params(**kw)
    _check(load_library().aa_quad_simplex_spg_batch(
        device_index(), _ptr(A), _ptr(B), sj, st, _ptr(Z0), _ptr(Z), n, k, ctypes.byref(p),
        iters.ctypes.data_as(_ip)))
    return (Z, iters) if return_iters else Z


def qp_kernels(ctx=None):
    """What the last per-sample QP launched, e.g. ``"k_qp_quad_w3<2,1,0>:cap=24;k_qp_wave<32,1,1>"``
    (aa_qp_kernels): of ``ctx``, or of the scratch context behind ``qp_batch`` on this device."""
    buf = ctypes.create_string_buffer(256)
    _check(load_library().aa_qp_kernels(None if ctx is None else ctx.h, device_index(), buf, 256))
    return buf.value.decode()


# ---------------------------------------------------------------- resident solver
class Context(object):
    """RAII wrapper of aa_ctx.  Use as a context manager."""

    def __init__(self, dtype=None, device=None):
        require_gpu()
        self.lib = load_library()
        self.h = _vp()
        self.dtype_code = dtype_code(dtype)
        self.device = device_index() if device is None else device
        _check(self.lib.aa_ctx_create(ctypes.byref(self.h), self.device, self.dtype_code))
        self.k = 0
        self.n = 0
        self.p = 0
        self.world = 1
        self.reused = 0            # fits served from the resident copy of the data (resident_context)
        # row shard of a distributed fit (sharded_context): with `global_view` the factor methods
        # below take and return arrays of the WHOLE problem and slice / gather this rank's rows
        self.global_view = False
        self.implicit = False      # an implicit kernel (set_rbf_features, set_poly_features): no stored matrix behind the products
        self.row_lo = 0
        self.n_global = 0
        self._data_owner = None    # the context whose matrix this one aliases (share_data): kept alive
        self._reference_kind = "rbf"   # the kind of the latest reference set (kernel_cross; the library refuses without one)

    def _adopt(self, n, p, row_lo=0, n_global=None, implicit=False, owner=None):
        """What an install left in the library (include/aa_hip.h, "installing data"); every setter of
        the data calls this once, after the library call has succeeded."""
        self.n, self.p = int(n), int(p)
        self.row_lo, self.n_global = int(row_lo), int(n if n_global is None else n_global)
        self.implicit = implicit
        self._data_owner = owner

    def close(self):
        if self.h:
            self.lib.aa_ctx_destroy(self.h)
            self.h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- comm
    def comm_init(self, unique_id, rank, world):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        _check(self.lib.aa_ctx_comm_init(self.h, ctypes.cast(buf, _vp), rank, world))
        self.world = world

    def p2p_init(self, rank, world, tag="fit"):
        """The one-shot peer-to-peer all-reduce as this context's transport (aa_ctx_p2p_*): the IPC
        handles of the ranks' receive buffers travel through files of the launch, like the RCCL
        unique id.  No RCCL involved; the ranks may even share a GPU."""
        mine = ctypes.create_string_buffer(64)
        _check(self.lib.aa_ctx_p2p_export(self.h, int(world), ctypes.cast(mine, _vp)))
        handles, paths = exchange_blobs(rank, world, mine.raw, "p2p_" + tag)
        buf = ctypes.create_string_buffer(b"".join(handles), 64 * world)
        _check(self.lib.aa_ctx_p2p_init(self.h, ctypes.cast(buf, _vp), int(rank), int(world)))
        self._p2p_paths = paths
        self.allreduce_host([0.0])               # everybody has opened everybody's buffer before the files go
        if rank == 0:
            for path in paths:
                try:
                    os.remove(path)
                except OSError:
                    pass

    def allreduce_host(self, values, op="sum"):
        a = _c64(np.atleast_1d(values)).copy()
        _check(self.lib.aa_ctx_allreduce_host(self.h, _ptr(a), a.size, 1 if op == "max" else 0))
        return a

    # -- data / state
    def set_data(self, X, form=FORM_DATA, n_global=None, row_offset=0):
        X = np.asarray(X)
        if X.dtype == np.float32:
            host = AA_F32
        else:
            X = np.asarray(X, dtype=np.float64)
            host = AA_F64
        X = np.ascontiguousarray(X)
        n, p = X.shape
        _check(self.lib.aa_set_data(self.h, X.ctypes.data_as(_vp), host, n, p, p, form,
                                    n if n_global is None else n_global, row_offset))
        self._adopt(n, p, row_offset, n_global)

    def _rows(self, a):
        """This rank's rows of a whole-problem array (global view only)."""
        return a[self.row_lo:self.row_lo + self.n] if self.global_view else a

    def _gather_rows(self, local):
        """Whole-problem array from every rank's rows: zero-padded sum all-reduce (exact: every
        entry is one value plus zeros)."""
        if not self.global_view:
            return local
        local = np.asarray(local, dtype=np.float64)
        full = np.zeros((self.n_global,) + local.shape[1:])
        full[self.row_lo:self.row_lo + self.n] = local
        flat = full.reshape(-1)
        step = 1 << 24                                    # aa_ctx_allreduce_host counts with an int
        for i in range(0, flat.size, step):
            flat[i:i + step] = self.allreduce_host(flat[i:i + step])
        return full

    def share_data(self, owner):
        """Use ``owner``'s resident data matrix without a copy (aa_share_data); ``owner`` must stay
        open while this context uses it."""
        _check(self.lib.aa_share_data(self.h, owner.h))
        self._adopt(owner.n, owner.p, owner.row_lo, owner.n_global, owner=owner)

    def set_data_rows(self, owner, row0, n):
        """Rows [row0, row0 + n) of ``owner``'s resident data matrix become this context's data matrix
        (aa_set_data_rows): a device-to-device copy that owns its memory."""
        _check(self.lib.aa_set_data_rows(self.h, owner.h, int(row0), int(n)))
        self._adopt(n, owner.p)

    def set_data_rows_affine(self, owner, row0, n, shift=None, scale=None):
        """``(owner[row0:row0 + n] - shift) / scale`` becomes this context's data matrix
        (aa_set_data_rows_affine): float64 arithmetic, one rounding to the context's dtype.  ``shift`` /
        ``scale``: None (0 / 1) or one value per column of ``owner``."""
        def column_values(a, name):
            if a is None:
                return None
            a = _c64(a)
            if a.shape != (owner.p,):
                raise ValueError("%s: %d values expected, one per column; got shape %r" % (name, owner.p, a.shape))
            return a
        shift, scale = column_values(shift, "shift"), column_values(scale, "scale")
        _check(self.lib.aa_set_data_rows_affine(self.h, owner.h, int(row0), int(n),
                                                None if shift is None else _ptr(shift),
                                                None if scale is None else _ptr(scale)))
        self._adopt(n, owner.p)

    def set_data_rows_model(self, owner, row0, n, groups=None, shift=None, intercept=None, slope=None, t=None,
                            scale=None):
        """``((owner[row0:row0 + n] - shift[groups]) - (intercept + slope * t[:, None])) / scale[groups]`` becomes
        this context's data matrix (aa_set_data_rows_model): the float64 roundings of that NumPy expression, one
        rounding to the context's dtype.  ``shift`` / ``scale``: None (part left out) or ``(G, p)`` tables, row
        ``groups[r]`` for row ``r`` of the block (``groups``: n integers in ``[0, G)``; None with ``G == 1``);
        ``intercept`` / ``slope``: one value per column, ``t``: one per row, all three or none."""
        n = int(n)
        tables = [None if a is None else np.atleast_2d(_c64(a)) for a in (shift, scale)]
        G = max([1] + [a.shape[0] for a in tables if a is not None])
        for a, name in zip(tables, ("shift", "scale")):
            if a is not None and a.shape != (G, owner.p):
                raise ValueError("%s: a (%d, %d) table expected, one row per group; got shape %r"
                                 % (name, G, owner.p, a.shape))
        trend = [None if a is None else _c64(a) for a in (intercept, slope, t)]
        if any(a is None for a in trend) != all(a is None for a in trend):
            raise ValueError("intercept, slope and t come together or not at all")
        for a, name, size in zip(trend, ("intercept", "slope", "t"), (owner.p, owner.p, n)):
            if a is not None and a.shape != (size,):
                raise ValueError("%s: %d values expected; got shape %r" % (name, size, a.shape))
        if groups is not None:
            groups = np.ascontiguousarray(groups, dtype=np.intc)
            if groups.shape != (n,):
                raise ValueError("groups: %d labels expected, one per row; got shape %r" % (n, groups.shape))
        ptr = [None if a is None else _ptr(a) for a in tables + trend]
        _check(self.lib.aa_set_data_rows_model(self.h, owner.h, int(row0), n, G,
                                               None if groups is None else groups.ctypes.data_as(_ip),
                                               ptr[0], ptr[2], ptr[3], ptr[4], ptr[1]))
        self._adopt(n, owner.p)

    def set_data_rows_slots(self, owner, row0, n, slots, shift=None, scale=None):
        """``(owner[row0:row0 + n] - shift[slots]) / scale[slots]`` becomes this context's data matrix
        (aa_set_data_rows_slots): the float64 roundings of that NumPy expression, one rounding to the context's
        dtype.  ``slots``: n integers in ``[0, G)``, one per row of the block; ``shift`` / ``scale``: ``(G, p)``
        tables, ``G <= MAX_SLOTS``, either may be None (part left out), not both.  Rows of the tables whose slot no
        row of the block uses are not read."""
        n = int(n)
        tables = [None if a is None else _c64(a) for a in (shift, scale)]
        if all(a is None for a in tables):
            raise ValueError("a shift table, a scale table or both are needed")
        G = max(a.shape[0] if a.ndim == 2 else 0 for a in tables if a is not None)
        for a, name in zip(tables, ("shift", "scale")):
            if a is not None and (a.ndim != 2 or a.shape != (G, owner.p)):
                raise ValueError("%s: a (%d, %d) table expected, one row per slot; got shape %r"
                                 % (name, G, owner.p, a.shape))
        slots = np.ascontiguousarray(slots, dtype=np.intc)
        if slots.shape != (n,):
            raise ValueError("slots: %d labels expected, one per row; got shape %r" % (n, slots.shape))
        ptr = [None if a is None else _ptr(a) for a in tables]
        _check(self.lib.aa_set_data_rows_slots(self.h, owner.h, int(row0), n, G, slots.ctypes.data_as(_ip),
                                               ptr[0], ptr[1]))
        self._adopt(n, owner.p)

    def set_data_take(self, owner, indices=None):
        """Rows ``indices`` (any order, duplicates allowed; None: all rows in order) of ``owner``'s resident data
        matrix become this context's data matrix (aa_set_data_take): a device gather that owns its memory.  A
        float32 owner widens exactly into a float64 context.  The library checks every index on the host before
        it launches anything (error -1, this context keeps its data)."""
        if indices is None:
            n, ptr = owner.n, None
        else:
            idx = np.ascontiguousarray(indices, dtype=np.int64)
            if idx.ndim != 1:
                raise ValueError("a 1-D index array expected; got shape %r" % (idx.shape,))
            n, ptr = idx.shape[0], idx.ctypes.data_as(ctypes.POINTER(ctypes.c_long))
        _check(self.lib.aa_set_data_take(self.h, owner.h, ptr, int(n)))
        self._adopt(n, owner.p)

    # -- implicit kernels: 'rbf' exp(-gamma ||x - y||^2) and 'poly' (gamma x.y + coef0)^degree, never formed.  The
    # library has one entry point per kind and operation (aa_set_<kind>_features, ..._features_resident,
    # aa_set_<kind>_reference, aa_<kind>_cross); _kernel_call picks it and appends the kind's parameters
    _KERNEL_NAMES = {"rbf": "RBF", "poly": "polynomial"}

    def _kernel_call(self, entry, kind, gamma, coef0, degree, *args):
        params = (float(gamma),) if kind == "rbf" else (float(gamma), float(coef0), int(degree))
        _check(getattr(self.lib, entry % kind)(self.h, *(args + params)))

    def _set_kernel_features(self, kind, gamma, coef0, degree, X=None, owner=None):
        """The implicit kernel of the rows of ``X`` (host), or of ``owner``'s resident data matrix (nothing
        crosses the bus; ``owner`` is only read), as this context's kernel matrix: kernel form, float64."""
        if owner is None:
            X = _c64(X)
            if X.ndim != 2:
                raise ValueError("feature matrix must be 2-D")
        if self.dtype_code != AA_F64:
            raise ValueError("the implicit %s kernel needs a float64 context" % self._KERNEL_NAMES[kind])
        if owner is None:
            n, p = X.shape
            self._kernel_call("aa_set_%s_features", kind, gamma, coef0, degree, _ptr(X), n, p, p)
        else:
            n = owner.n
            self._kernel_call("aa_set_%s_features_resident", kind, gamma, coef0, degree, owner.h)
        self._adopt(n, n, implicit=True)

    def set_rbf_features(self, X, gamma):
        self._set_kernel_features("rbf", gamma, 0.0, 1, X=X)

    def set_poly_features(self, X, gamma, coef0, degree):
        self._set_kernel_features("poly", gamma, coef0, degree, X=X)

    def set_rbf_features_resident(self, owner, gamma):
        self._set_kernel_features("rbf", gamma, 0.0, 1, owner=owner)

    def set_poly_features_resident(self, owner, gamma, coef0, degree):
        self._set_kernel_features("poly", gamma, coef0, degree, owner=owner)

    @staticmethod
    def _spec_args(spec):
        """``(kind, gamma, coef0, degree)`` of a kernel dict ``dict(form=, gamma=[, coef0=, degree=])``."""
        return spec["form"], spec["gamma"], spec.get("coef0", 0.0), spec.get("degree", 1)

    def set_kernel_features(self, spec, X_or_owner):
        """set_<form>_features[_resident] for the kernel ``spec`` names (KernelAA's ``_kernel_spec``); a
        ``Context`` as the second argument is an owner."""
        key = "owner" if isinstance(X_or_owner, type(self)) else "X"
        self._set_kernel_features(*self._spec_args(spec), **{key: X_or_owner})

    def data_column_moments(self, mean=True, var=True):
        """``(mean[p], var[p])`` of the columns of the resident data matrix (aa_data_column_moments): two
        float64 sweeps, ``var`` the mean squared deviation (ddof 0); an output that is not asked for is None."""
        m = np.empty(self.p) if mean else None
        v = np.empty(self.p) if var else None
        _check(self.lib.aa_data_column_moments(self.h, None if m is None else _ptr(m), None if v is None else _ptr(v)))
        return m, v

    def data_weighted_column_sums(self, A, groups=None, centre=None):
        """``A @ X`` for the resident data matrix ``X`` and a ``(G, n)`` coefficient matrix, ``G <= 16``
        (aa_data_weighted_column_sums), or with ``groups`` (n integers, -1: row not counted) and a ``(Gc, p)``
        table ``centre``: ``out[g] = sum_t A[g, t] * (X[t] - centre[groups[t]]) ** 2`` (aa_data_grouped_sqdev).
        float64 arithmetic and a fixed summation order in both context dtypes.  Returns ``(G, p)`` float64."""
        A = _c64(A)
        if A.ndim != 2 or A.shape[1] != self.n:
            raise ValueError("a (G, %d) coefficient matrix expected, one column per resident row; got shape %r"
                             % (self.n, A.shape))
        out = np.empty((A.shape[0], self.p))
        if centre is None and groups is None:
            _check(self.lib.aa_data_weighted_column_sums(self.h, A.shape[0], _ptr(A), _ptr(out)))
            return out
        if centre is None or groups is None:
            raise ValueError("groups and centre come together")
        centre = _c64(centre)
        groups = np.ascontiguousarray(groups, dtype=np.intc)
        if centre.ndim != 2 or centre.shape[1] != self.p:
            raise ValueError("centre: a (Gc, %d) table expected; got shape %r" % (self.p, centre.shape))
        if groups.shape != (self.n,):
            raise ValueError("groups: %d labels expected, one per row; got shape %r" % (self.n, groups.shape))
        _check(self.lib.aa_data_grouped_sqdev(self.h, A.shape[0], _ptr(A), groups.ctypes.data_as(_ip), _ptr(centre),
                                              centre.shape[0], _ptr(out)))
        return out

    def data_slot_sums(self, slots, n_slots, centre=None):
        """``(sums, counts)`` of the resident data matrix per calendar slot (aa_data_slot_sums): ``sums[g] = sum of
        X[t]`` over the rows with ``slots[t] == g``, or of ``(X[t] - centre[g]) ** 2`` with a ``(n_slots, p)`` table
        ``centre``; ``slots``: n integers in ``[-1, n_slots)``, -1: row not counted; ``n_slots <= MAX_SLOTS``.
        float64 arithmetic and a fixed summation order in both context dtypes.  A slot without counted rows has sums
        exactly 0 and count 0, and its row of ``centre`` is not read.  Returns ``(n_slots, p)`` float64 and
        ``(n_slots,)`` int64."""
        G = int(n_slots)
        slots = np.ascontiguousarray(slots, dtype=np.intc)
        if slots.shape != (self.n,):
            raise ValueError("slots: %d labels expected, one per row; got shape %r" % (self.n, slots.shape))
        if centre is not None:
            centre = _c64(centre)
            if centre.shape != (G, self.p):
                raise ValueError("centre: a (%d, %d) table expected; got shape %r" % (G, self.p, centre.shape))
        out = np.empty((max(G, 0), self.p))
        counts = np.zeros(max(G, 0), dtype=np.int64)
        _check(self.lib.aa_data_slot_sums(self.h, G, slots.ctypes.data_as(_ip), None if centre is None else _ptr(centre),
                                          _ptr(out), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_long))))
        return out, counts

    def data_gram(self, side, shift=None):
        """The Gram matrix of the resident data matrix, centred by ``shift`` (one value per column; None: not
        centred), with itself (aa_data_gram): ``side='rows'`` -- ``Xc @ Xc.T`` (n, n); ``'cols'`` -- ``Xc.T @ Xc``
        (p, p).  float64 on the f64 matrix cores in both context dtypes, exactly symmetric, the same bits on every
        call; the side's size is at most ``GRAM_MAX_D``."""
        if side not in GRAM_SIDES:
            raise ValueError("side must be one of %r; got %r" % (GRAM_SIDES, side))
        if shift is not None:
            shift = _c64(shift)
            if shift.shape != (self.p,):
                raise ValueError("shift: %d values expected, one per column; got shape %r" % (self.p, shift.shape))
        d = self.n if side == "rows" else self.p
        out = np.empty((d, d))
        _check(self.lib.aa_data_gram(self.h, GRAM_SIDES.index(side), None if shift is None else _ptr(shift),
                                     _ptr(out), d))
        return out

    def set_data_projected(self, owner, row0, n, V, shift=None):
        """``(owner[row0:row0 + n] - shift) @ V.T`` becomes this context's data matrix (aa_set_data_projected):
        ``V`` is ``(q, p)``, ``q <= MAX_PROJECTED``; float64 sums on the f64 matrix cores, one rounding to this
        context's dtype.  A float32 owner may feed a float64 context."""
        V = _c64(V)
        if V.ndim != 2 or V.shape[1] != owner.p:
            raise ValueError("V: a (q, %d) matrix expected, one column per column of the owner; got shape %r"
                             % (owner.p, V.shape))
        if shift is not None:
            shift = _c64(shift)
            if shift.shape != (owner.p,):
                raise ValueError("shift: %d values expected, one per column; got shape %r" % (owner.p, shift.shape))
        _check(self.lib.aa_set_data_projected(self.h, owner.h, int(row0), int(n), V.shape[0], _ptr(V), V.shape[1],
                                              None if shift is None else _ptr(shift)))
        self._adopt(n, V.shape[0])

    def set_linear_kernel(self, on):
        """The resident data matrix X stands in for the kernel K = X X' of KernelAA
        (aa_set_linear_kernel): kernel-form conventions, K never formed."""
        _check(self.lib.aa_set_linear_kernel(self.h, 1 if on else 0))

    def set_data_weighted(self, raw, col_weights=None, row0=0, n=None):
        """Driver preprocessing on the device (aa_set_data_weighted): ``raw`` is the flattened
        n_total x p_full field with NaN for missing values; returns the boolean mask of the
        columns kept (no NaN in any row).  Rows [row0, row0 + n) become the data matrix."""
        raw = np.asarray(raw)
        if raw.dtype == np.float32:
            host = AA_F32
        else:
            raw = np.asarray(raw, dtype=np.float64)
            host = AA_F64
        raw = np.ascontiguousarray(raw)
        n_total, p_full = raw.shape
        n = n_total - row0 if n is None else n
        w = None if col_weights is None else _c64(np.broadcast_to(col_weights, (p_full,)))
        valid = np.zeros(p_full, dtype=np.uint8)
        pv = ctypes.c_long(0)
        _check(self.lib.aa_set_data_weighted(
            self.h, raw.ctypes.data_as(_vp), host, n_total, p_full, p_full, None if w is None else _ptr(w),
            int(row0), int(n), valid.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), ctypes.byref(pv)))
        self._adopt(n, pv.value)
        return valid.astype(bool)

    def get_data(self):
        out = np.empty((self.n, self.p))
        _check(self.lib.aa_get_data(self.h, _ptr(out), self.p))
        return out

    def data_trace(self):
        t = ctypes.c_double(0)
        _check(self.lib.aa_data_trace(self.h, ctypes.byref(t)))
        return t.value

    def set_state(self, C, Z, alpha):
        if self.global_view:
            C, Z = np.asarray(C)[:, self.row_lo:self.row_lo + self.n], self._rows(np.asarray(Z))
        C, Z, alpha = _c64(C), _c64(Z), _c64(alpha)
        k = C.shape[0]
        _check(self.lib.aa_set_state(self.h, k, _ptr(C), C.shape[1], _ptr(Z), _ptr(alpha)))
        self.k = k

    def get_state(self):
        C = np.empty((self.k, self.n))
        Z = np.empty((self.n, self.k))
        alpha = np.empty(self.k)
        _check(self.lib.aa_get_state(self.h, _ptr(C), self.n, _ptr(Z), _ptr(alpha)))
        if self.global_view:
            C = np.ascontiguousarray(self._gather_rows(np.ascontiguousarray(C.T)).T)
            Z = self._gather_rows(Z)
        return C, Z, alpha

    def set_alpha(self, alpha):
        alpha = _c64(alpha)
        _check(self.lib.aa_set_alpha(self.h, _ptr(alpha)))

    def prepare(self):
        c = ctypes.c_double(0)
        _check(self.lib.aa_prepare(self.h, ctypes.byref(c)))
        return c.value

    def cost(self):
        c = ctypes.c_double(0)
        _check(self.lib.aa_cost(self.h, ctypes.byref(c)))
        return c.value

    def grams(self):
        k = self.k
        ZtZ, CKCt, CKZ = np.empty((k, k)), np.empty((k, k)), np.empty((k, k))
        t = ctypes.c_double(0)
        _check(self.lib.aa_get_grams(self.h, _ptr(ZtZ), _ptr(CKCt), _ptr(CKZ), ctypes.byref(t)))
        return ZtZ, CKCt, CKZ, t.value

    def set_dictionary_inputs(self, KZ, ZtZ, trace):
        KZ, ZtZ = _c64(KZ), _c64(ZtZ)
        _check(self.lib.aa_set_dictionary_inputs(self.h, _ptr(KZ), _ptr(ZtZ), float(trace)))

    def dictionary_update(self, **spg_kw):
        p = spg_params(**spg_kw)
        st = SPGStats()
        _check(self.lib.aa_dictionary_update(self.h, ctypes.byref(p), ctypes.byref(st)))
        return st

    def weights_update(self, **qp_kw):
        p = qp_params(**qp_kw)
        st = QPStats()
        _check(self.lib.aa_weights_update(self.h, ctypes.byref(p), ctypes.byref(st)))
        return st

    def outer_iterations(self, n_outer, spg_kw, qp_kw):
        sp, qp = spg_params(**spg_kw), qp_params(**qp_kw)
        costs = np.zeros(2 * n_outer)
        _check(self.lib.aa_outer_iterations(self.h, n_outer, ctypes.byref(sp), ctypes.byref(qp),
                                            _ptr(costs)))
        return costs

    def outer_iterations_nocost(self, n_outer, spg_kw, qp_kw):
        """The same iterations without a cost record (with the library option ``outer_nosync`` the
        call returns while the work is in flight: tools/interleave_probe.py)."""
        sp, qp = spg_params(**spg_kw), qp_params(**qp_kw)
        _check(self.lib.aa_outer_iterations(self.h, n_outer, ctypes.byref(sp), ctypes.byref(qp), None))

    def iterate(self, cost0, max_outer, tolerance, stopping_criterion, require_monotonic,
                update_dictionary, update_weights, spg_kw, qp_kw, check_every=8,
                mono_tolerance=None, delta=0.0, scale_kw=None):
        """Up to ``max_outer`` outer iterations with the monotonicity check and the stopping rule
        evaluated on the device (aa_iterate); returns (costs[2 * (n_iter + 1)], IterStats)."""
        ip = _iter_params(max_outer, tolerance, stopping_criterion, require_monotonic, mono_tolerance,
                          update_dictionary, update_weights, check_every, delta)
        sp, qp = spg_params(**spg_kw), qp_params(**qp_kw)
        ssp = spg_params(**scale_kw) if (scale_kw is not None and delta != 0) else None
        costs = np.zeros(2 * int(max_outer))
        st = IterStats()
        _check(self.lib.aa_iterate(self.h, ctypes.byref(ip), ctypes.byref(sp), ctypes.byref(qp),
                                   None if ssp is None else ctypes.byref(ssp),
                                   float(cost0), _ptr(costs), ctypes.byref(st)))
        return costs[:2 * (st.n_iter + 1)], st

    def reconstruction_cost(self):
        c = ctypes.c_double(0)
        _check(self.lib.aa_reconstruction_cost(self.h, ctypes.byref(c)))
        return c.value

    def archetypes(self):
        out = np.empty((self.k, self.p))
        _check(self.lib.aa_get_archetypes(self.h, _ptr(out), self.p))
        return out

    def distance_column(self, j):
        d = np.empty(self.n)
        _check(self.lib.aa_distance_column(self.h, int(j), _ptr(d)))
        return self._gather_rows(d)

    def furthest_sum(self, n_components, start_index, exclude=None, extra_steps=1):
        """FurthestSum on the device (aa_furthest_sum); returns the selected indices, or None when a
        pick met a shared maximum (the caller then uses the host's list logic) or the context is
        row-sharded."""
        if self.global_view or self.implicit or n_components < 1 or n_components > MAX_K:
            return None
        ex = np.ascontiguousarray([] if exclude is None else exclude, dtype=np.int32)
        sel = np.zeros(int(n_components), dtype=np.int32)
        tie = ctypes.c_int(0)
        _check(self.lib.aa_furthest_sum(self.h, int(n_components), int(start_index),
                                        ex.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(ex.size),
                                        int(max(extra_steps, 0)),
                                        sel.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(tie)))
        return None if tie.value else sel.astype(np.int64)

    def furthest_sum_state(self):
        """What the latest ``furthest_sum`` left on the device (aa_get_furthest_sum_state): a dict with ``sums``
        (n), ``alive`` (n, bool), ``column`` (n: the last distance column of the chain), ``cur``, ``tie`` and
        ``selected`` (k).  Raises when no selection has run since the data was installed."""
        n, k = ctypes.c_long(0), ctypes.c_int(0)
        _check(self.lib.aa_get_furthest_sum_state(self.h, ctypes.byref(n), ctypes.byref(k), None, None, None,
                                                  None, None, None))
        sums, column = np.empty(n.value), np.empty(n.value)
        alive = np.empty(n.value, dtype=np.uint8)
        selected = np.zeros(k.value, dtype=np.int32)
        cur, tie = ctypes.c_int(0), ctypes.c_int(0)
        _check(self.lib.aa_get_furthest_sum_state(self.h, None, None, _ptr(sums),
                                                  alive.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), _ptr(column),
                                                  ctypes.byref(cur), ctypes.byref(tie),
                                                  selected.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return dict(sums=sums, alive=alive.astype(bool), column=column, cur=cur.value, tie=tie.value,
                    selected=selected.astype(np.int64))

    # -- GPNH
    def gpnh_set_factors(self, k, W=None, Z=None):
        """W is the reference's dictionary (p x k); it travels transposed (k x p)."""
        Wt = None if W is None else _c64(np.asarray(W).T)
        Zc = None if Z is None else _c64(self._rows(np.asarray(Z)))
        _check(self.lib.aa_gpnh_set_factors(self.h, k, None if Wt is None else _ptr(Wt), self.p,
                                            None if Zc is None else _ptr(Zc)))
        self.k = k

    def gpnh_get_weights(self):
        Z = np.empty((self.n, self.k))
        _check(self.lib.aa_gpnh_get_weights(self.h, _ptr(Z)))
        return self._gather_rows(Z)

    def gpnh_reduce(self, want_ztx=True, want_trace=True):
        k = self.k
        ZtX = np.empty((k, self.p)) if want_ztx else None
        ZtZ = np.empty((k, k))
        tr = ctypes.c_double(0)
        _check(self.lib.aa_gpnh_reduce(self.h, None if ZtX is None else _ptr(ZtX), self.p, _ptr(ZtZ),
                                       ctypes.byref(tr) if want_trace else None))
        return ZtX, ZtZ, tr.value

    def gpnh_weights_update(self, WtW, **qp_kw):
        WtW = _c64(WtW)
        p = qp_params(**qp_kw)
        st = QPStats()
        _check(self.lib.aa_gpnh_weights_update(self.h, _ptr(WtW), ctypes.byref(p), ctypes.byref(st)))
        return st

    def gpnh_iterate(self, lambda_W, max_outer, tolerance, stopping_criterion, require_monotonic,
                     update_dictionary, update_weights, qp_kw, check_every=8, mono_tolerance=None):
        """The GPNH alternating loop on the device (aa_gpnh_iterate); returns
        (cost0, costs[2 * (n_iter + 1)], IterStats).  stats.error_stage == 3: the regularised
        normal equations were not positive definite (the caller falls back to lstsq)."""
        gp = GPNHParams(float(lambda_W), _iter_params(max_outer, tolerance, stopping_criterion, require_monotonic,
                                                      mono_tolerance, update_dictionary, update_weights,
                                                      check_every, 0.0))
        qp = qp_params(**qp_kw)
        costs = np.zeros(2 * int(max_outer))
        st = IterStats()
        c0 = ctypes.c_double(0)
        _check(self.lib.aa_gpnh_iterate(self.h, ctypes.byref(gp), ctypes.byref(qp), ctypes.byref(c0),
                                        _ptr(costs), ctypes.byref(st)))
        return c0.value, costs[:2 * (max(st.n_iter, -1) + 1)], st

    # ---- GPNH restarts side by side (aa_gpnh_slots_*; restarts.fit_restarts drives them)
    def gpnh_slots_begin(self, n_slots, k, lambda_W, max_outer, tolerance, stopping_criterion, require_monotonic,
                         qp_kw, mono_tolerance=None):
        gp = GPNHParams(float(lambda_W), _iter_params(max_outer, tolerance, stopping_criterion, require_monotonic,
                                                      mono_tolerance, True, True, 8, 0.0))
        qp = qp_params(**qp_kw)
        _check(self.lib.aa_gpnh_slots_begin(self.h, int(n_slots), int(k), ctypes.byref(gp), ctypes.byref(qp)))
        self.k = int(n_slots) * int(k)
        self._slots = (int(n_slots), int(k), int(max_outer))

    def gpnh_slots_load(self, r, W, Z):
        """``W``: n_features x k (the reference's dictionary layout), ``Z``: n_samples x k."""
        Wt = _c64(np.asarray(W).T)
        Z = _c64(Z)
        _check(self.lib.aa_gpnh_slots_load(self.h, int(r), _ptr(Wt), Wt.shape[1], _ptr(Z)))

    def _slots_run(self, fn, n_iters):
        st = (SlotStatus * self._slots[0])()
        _check(fn(self.h, int(n_iters), st))
        return list(st)

    def gpnh_slots_run(self, n_iters):
        return self._slots_run(self.lib.aa_gpnh_slots_run, n_iters)

    def gpnh_slots_fetch(self, r, stop_iter):
        """(weights n x k, dictionary p x k, cost0, costs[2 (stop_iter + 1)]) of a stopped slot."""
        _, k, _ = self._slots
        Wt = np.empty((k, self.p))
        Z = np.empty((self.n, k))
        costs = np.zeros(2 * (int(stop_iter) + 1))
        c0 = ctypes.c_double(0)
        _check(self.lib.aa_gpnh_slots_fetch(self.h, int(r), _ptr(Wt), self.p, _ptr(Z), _ptr(costs), ctypes.byref(c0)))
        return Z, Wt.T, c0.value, costs

    # ---- AA restarts side by side (aa_slots_*)
    def aa_slots_begin(self, n_slots, k, max_outer, tolerance, stopping_criterion, require_monotonic, spg_kw, qp_kw,
                       mono_tolerance=None, delta=0.0, scale_kw=None):
        ip = _iter_params(max_outer, tolerance, stopping_criterion, require_monotonic, mono_tolerance, True, True, 8,
                          delta)
        sp, qp = spg_params(**spg_kw), qp_params(**qp_kw)
        scale = spg_params(**(scale_kw or {})) if delta != 0 else None
        _check(self.lib.aa_slots_begin(self.h, int(n_slots), int(k), ctypes.byref(ip), ctypes.byref(sp),
                                       ctypes.byref(qp), ctypes.byref(scale) if scale is not None else None))
        self.k = int(n_slots) * int(k)
        self._slots = (int(n_slots), int(k), int(max_outer))

    def _aa_slots_put(self, fn, r, C, Z, alpha):
        C, Z = _c64(C), _c64(Z)
        a = None if alpha is None else _c64(alpha)
        _check(fn(self.h, int(r), _ptr(C), C.shape[1], _ptr(Z), None if a is None else _ptr(a)))

    def aa_slots_load(self, r, C, Z, alpha=None):
        """``C``: k x n_samples, ``Z``: n_samples x k, into slot r of a group that has not run yet."""
        self._aa_slots_put(self.lib.aa_slots_load, r, C, Z, alpha)

    def aa_slots_reload(self, r, C, Z, alpha=None):
        """The same into a freed slot of a RUNNING group (the other slots carry on)."""
        self._aa_slots_put(self.lib.aa_slots_reload, r, C, Z, alpha)

    def aa_slots_run(self, n_iters):
        return self._slots_run(self.lib.aa_slots_run, n_iters)

    def aa_slots_fetch(self, r, stop_iter, carried):
        """(weights n x k, dictionary k x n, C X k x p, cost0, costs[2 (stop_iter + 1)], alpha[k]) of a stopped slot."""
        _, k, _ = self._slots
        C = np.empty((k, self.n))
        Z = np.empty((self.n, k))
        CX = np.empty((k, self.p))
        alpha = np.ones(k)
        costs = np.zeros(2 * (int(stop_iter) + 1))
        c0 = ctypes.c_double(0)
        _check(self.lib.aa_slots_fetch(self.h, int(r), _ptr(C), self.n, _ptr(Z), _ptr(CX), self.p, int(bool(carried)),
                                       _ptr(costs), ctypes.byref(c0), _ptr(alpha)))
        return Z, C, CX, c0.value, costs, alpha

    def aa_slots_end(self):
        _check(self.lib.aa_slots_end(self.h))
        self._slots = None

    def gpnh_get_dictionary(self):
        """The reference's dictionary (p x k, returned like the reference returns it: the
        transpose of a C-ordered k x p array)."""
        Wt = np.empty((self.k, self.p))
        _check(self.lib.aa_gpnh_get_dictionary(self.h, _ptr(Wt), self.p))
        return Wt.T

    def gpnh_residual_cost(self):
        c = ctypes.c_double(0)
        _check(self.lib.aa_gpnh_residual_cost(self.h, ctypes.byref(c)))
        return c.value

    def gpnh_residual_scores(self, columns=True, samples=True, total=True):
        """Sums of squares of R = X - Z W' on the resident matrix in one pass (aa_gpnh_residual_scores):
        ``(column_sse[p], sample_sse[n], sse)``; an output that is not asked for is None."""
        col = np.empty(self.p) if columns else None
        row = np.empty(self.n) if samples else None
        tot = ctypes.c_double(0)
        _check(self.lib.aa_gpnh_residual_scores(self.h, None if col is None else _ptr(col),
                                                None if row is None else _ptr(row),
                                                ctypes.byref(tot) if total else None))
        return col, row, (tot.value if total else None)

    # -- KernelAA.transform (aa_set_rbf_reference / aa_rbf_cross, aa_set_poly_reference / aa_poly_cross,
    # aa_kernel_transform_cost)
    def _set_kernel_reference(self, kind, gamma, coef0, degree, XS, V):
        """Reference set of the cross kernel product for the resident rows Y (set_data): the training rows
        ``XS`` (s x p) and ``V`` (s x k, = D' on them).  Sizes the factor buffers for k components."""
        XS, V = _c64(XS), _c64(V)
        if XS.ndim != 2 or V.ndim != 2 or V.shape[0] != XS.shape[0]:
            raise ValueError("reference rows (s x p) and V (s x k) expected")
        s, p = XS.shape
        k = V.shape[1]
        self._kernel_call("aa_set_%s_reference", kind, gamma, coef0, degree, int(k), _ptr(XS), s, p, p, _ptr(V), k)
        self.k = k
        self._reference_kind = kind

    def _kernel_cross(self, kind, fetch):
        """XW = kappa(Y, XS) V into the QP's linear-term buffer (what gpnh_weights_update reads); with
        ``fetch`` also returned (m x k)."""
        out = np.empty((self.n, self.k)) if fetch else None
        _check(getattr(self.lib, "aa_%s_cross" % kind)(self.h, None if out is None else _ptr(out)))
        return out

    def set_rbf_reference(self, XS, V, gamma):
        self._set_kernel_reference("rbf", gamma, 0.0, 1, XS, V)

    def set_poly_reference(self, XS, V, gamma, coef0, degree):
        self._set_kernel_reference("poly", gamma, coef0, degree, XS, V)

    def rbf_cross(self, fetch=False):
        return self._kernel_cross("rbf", fetch)

    def poly_cross(self, fetch=False):
        return self._kernel_cross("poly", fetch)

    def set_kernel_reference(self, spec, XS, V):
        self._set_kernel_reference(*(self._spec_args(spec) + (XS, V)))

    def kernel_cross(self, fetch=False):
        """The cross product of the kernel the latest set_kernel_reference named."""
        return self._kernel_cross(self._reference_kind, fetch)

    def kernel_transform_cost(self, A, diag=None):
        """0.5 sum_t (d_t - 2 z_t.XW_t + z_t' A z_t) / m from the resident weights and linear terms;
        ``diag`` (m values) = kappa(y_t, y_t), None: 1 (RBF)."""
        A = _c64(A)
        d = None if diag is None else _c64(diag)
        c = ctypes.c_double(0)
        _check(self.lib.aa_kernel_transform_cost(self.h, _ptr(A), None if d is None else _ptr(d), ctypes.byref(c)))
        return c.value

    def kernel_sample_residuals(self, A, kind, diag=None, samples=True, diagonal=True):
        """The terms of kernel_transform_cost per sample (aa_kernel_sample_residuals):
        ``(r[n], d[n], sum r, sum d)`` with r_t = d_t - 2 z_t.XW_t + z_t' A z_t; ``kind`` one of ``DIAG_KINDS``
        ('given': d = ``diag``; 'ones'; 'poly': from the reference set's parameters; 'linear': |y_t|^2, both from
        row norms computed on the device).  A vector that is not asked for is None."""
        A = _c64(A)
        d = None if diag is None else _c64(diag)
        if d is not None and d.shape != (self.n,):
            raise ValueError("diag: %d values expected, one per resident row; got shape %r" % (self.n, d.shape))
        r = np.empty(self.n) if samples else None
        dout = np.empty(self.n) if diagonal else None
        sums = np.zeros(2)
        _check(self.lib.aa_kernel_sample_residuals(self.h, _ptr(A), DIAG_KINDS.index(kind),
                                                   None if d is None else _ptr(d), None if r is None else _ptr(r),
                                                   None if dout is None else _ptr(dout), _ptr(sums)))
        return r, dout, float(sums[0]), float(sums[1])

    def spg_scalars(self):
        """Scalar state of the latest dictionary SPG iteration (aa_get_spg_scalars), as a dict."""
        out = np.zeros(21)
        _check(self.lib.aa_get_spg_scalars(self.h, _ptr(out)))
        names = ("trace", "s1", "a0", "f_old", "f_new", "alpha", "alpha_set", "lambda", "delta", "dd", "s1d",
                 "a1", "a2", "dgn", "res2", "resinf", "n_feval", "flags", "proj_a", "ainv", "fnorm")
        return dict(zip(names, out.tolist()))

    def pass_reduce_rows(self, A):
        """A' X for a host n x k array A through the reduce-over-rows pass kernel (k x p)."""
        A = _c64(A)
        k = A.shape[1]
        out = np.empty((k, self.p))
        _check(self.lib.aa_pass_reduce_rows(self.h, k, _ptr(A), _ptr(out), self.p))
        self.k = k
        return out

    def pass_reduce_rows_flagged(self, A):
        """``pass_reduce_rows`` through the path for an operand that is zero in most rows (option
        ``reduce_sparse``): the same bits for finite data."""
        A = _c64(A)
        k = A.shape[1]
        out = np.empty((k, self.p))
        _check(self.lib.aa_pass_reduce_rows_flagged(self.h, k, _ptr(A), _ptr(out), self.p))
        self.k = k
        return out

    def reduce_sparse_counts(self):
        """Row slabs of the latest flagged reduce-over-rows call: ``(gathered, dense)``."""
        out = (ctypes.c_long * 2)()
        _check(self.lib.aa_reduce_sparse_counts(self.h, out))
        return int(out[0]), int(out[1])

    def pass_row_local(self, B):
        """X B' for a host k x p array B through the row-local pass kernel (n x k)."""
        B = _c64(B)
        k = B.shape[0]
        out = np.empty((self.n, k))
        _check(self.lib.aa_pass_row_local(self.h, k, _ptr(B), B.shape[1], _ptr(out)))
        self.k = k
        return out

    def gemm_timing(self, enable):
        """Switch the in-context event timing of the two pass kernels on/off; returns
        (ms_reduce_rows, launches, ms_row_local, launches) recorded since the last call."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        na, nb = ctypes.c_int(0), ctypes.c_int(0)
        _check(self.lib.aa_gemm_timing(self.h, int(bool(enable)), ctypes.byref(a), ctypes.byref(na),
                                       ctypes.byref(b), ctypes.byref(nb)))
        return a.value, na.value, b.value, nb.value

    def pass_kernels(self):
        """(reduce-over-rows kernel, row-local kernel) of the most recent passes of this context:
        which kernels the shard size and dtype selected."""
        buf = ctypes.create_string_buffer(128)
        _check(self.lib.aa_pass_kernels(self.h, buf, 128))
        return tuple(buf.value.decode().split(";"))

    def qp_kernels(self):
        """The kernels of the last weights QP of this context (see the module's ``qp_kernels``)."""
        return qp_kernels(self)

    def proj_counts(self):
        """Column simplex projections this context has launched so far, by strategy:
        ``{"small32", "small64", "list", "iterative"}`` (aa_proj_counts)."""
        out = (ctypes.c_long * 4)()
        _check(self.lib.aa_proj_counts(self.h, out))
        return dict(zip(("small32", "small64", "list", "iterative"), (int(v) for v in out)))

    SPG_ARRAYS = ("g", "g_prev", "d", "Gr", "Gr_prev", "H", "M", "Q", "f_mem")

    def spg_array(self, name):
        """One device array of the latest dictionary update (aa_get_spg_array): ``g``, ``g_prev``, ``d``,
        ``Gr``, ``Gr_prev``, ``H`` (n x k), ``M`` (k x k), ``Q`` (k x p, data form) or ``f_mem`` (16)."""
        shape = {"M": (self.k, self.k), "Q": (self.k, self.p), "f_mem": (16,)}.get(name, (self.n, self.k))
        out = np.empty(shape)
        _check(self.lib.aa_get_spg_array(self.h, self.SPG_ARRAYS.index(name), _ptr(out)))
        return out

    def spg_path(self):
        """Set-up and kernels of the latest dictionary update, in launch order (aa_spg_path), e.g.
        ``["cold", "k_grad<32>:nb=1:rpb=64", "k_gram_wide_pq_mfma<32>:nb=1:cpb=128", "k_linesearch_fin",
        "k_grad<32>:nb=1:rpb=64"]``."""
        buf = ctypes.create_string_buffer(512)
        _check(self.lib.aa_spg_path(self.h, buf, 512))
        return buf.value.decode().split(";")

    def time_kernel(self, which, reps):
        ms = ctypes.c_double(0)
        _check(self.lib.aa_time_kernel(self.h, which, reps, ctypes.byref(ms)))
        return ms.value


class borrowed(object):
    """``with borrowed(ctx) as ctx``: a context somebody else owns (not closed on exit)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        return False


# ---------------------------------------------------------------- data kept resident across fits
# The drivers fit the same matrix n_init = 100 times (bin/run_hadisst_aa.py:158-172,
# bin/run_jra55_pca_gpnh.py:123-136), each time through a fresh estimator.  Estimator instances
# hold no device handles (deepcopy-safe), so the context that owns the uploaded matrix is kept
# HERE, keyed on the host array: a restart with the same data finds it on the device and only
# sends its k x n / n x k start factors.  One entry; `release_device_cache()` frees it.
_resident = {"key": None, "ctx": None, "busy": False}
_resident_lock = threading.Lock()


def _digest(X):
    """Checksum of the WHOLE buffer (an in-place edit of any entry between two fits must not be
    served from the stale device copy).  xxh3 runs at memory speed (~0.15 s for the 1.6 GB
    headline matrix, against an upload of the same order); zlib.crc32 when xxhash is missing."""
    # (a uint8 view: memoryview.cast refuses non-native-endian and structured dtypes)
    buf = memoryview(np.ascontiguousarray(X).reshape(-1).view(np.uint8))
    try:
        import xxhash
        return xxhash.xxh3_64_intdigest(buf)
    except ImportError:
        return zlib.crc32(buf)


def _fingerprint(X, form, code, device):
    """Identity of a host matrix: buffer address, layout, and a checksum of every byte."""
    return (X.__array_interface__["data"][0], X.shape, X.strides, X.dtype.str, _digest(X), form, code, device)


class _Borrowed(object):
    """`with resident_context(...) as ctx`: leaving the block keeps the context alive and hands
    it back (one borrower at a time: a second thread gets a private context)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        with _resident_lock:
            if _resident["ctx"] is self.ctx:
                _resident["busy"] = False
        if exc[0] is not None:                    # a failed fit may leave the context inconsistent
            release_device_cache()
        return False


def resident_context(X, form=FORM_DATA, dtype=None, device=None):
    """Context with ``X`` loaded, reused from the previous fit of the same array (same buffer,
    shape, dtype, checksum of the whole buffer, form, arithmetic).  CONVEX_DIM_RED_CACHE=0
    switches the reuse off.  While one thread holds the resident context, other threads get a
    private context of their own (closed when their `with` block ends)."""
    X = np.asarray(X)
    code = dtype_code(dtype)
    dev = device_index() if device is None else device

    def private():
        ctx = Context(dtype=dtype, device=device)
        ctx.set_data(X, form=form)
        return ctx                                   # a plain context manager: closed on exit

    if os.environ.get("CONVEX_DIM_RED_CACHE", "1") == "0" or X.ndim != 2 or X.size == 0:
        return private()
    key = _fingerprint(X, form, code, dev)
    stale = None
    with _resident_lock:
        if _resident["busy"]:
            reuse = None
        elif _resident["key"] == key and _resident["ctx"] is not None and _resident["ctx"].h:
            _resident["busy"] = True
            _resident["ctx"].reused += 1
            return _Borrowed(_resident["ctx"])
        else:
            stale, _resident["key"], _resident["ctx"] = _resident["ctx"], None, None
            _resident["busy"] = True                 # reserved while the upload runs
            reuse = True
    if reuse is None:
        return private()
    if stale is not None:
        stale.close()
    try:
        ctx = Context(dtype=dtype, device=device)
        ctx.set_data(X, form=form)
    except Exception:
        with _resident_lock:
            _resident["busy"] = False
        raise
    ctx.reused = 0
    with _resident_lock:
        _resident["key"], _resident["ctx"] = key, ctx
    return _Borrowed(ctx)


def release_device_cache():
    """Free the data matrix kept on the device between fits."""
    with _resident_lock:
        ctx = _resident["ctx"]
        _resident["key"], _resident["ctx"], _resident["busy"] = None, None, False
    if ctx is not None:
        ctx.close()


atexit.register(release_device_cache)


def comm_transport():
    """'rccl' (default: ncclAllReduce over xGMI) or 'p2p' (AA_COMM=p2p: the one-shot peer-to-peer
    all-reduce of csrc/comm.hip, one kernel per rank and collective; single node, <= 8 ranks)."""
    v = os.environ.get("AA_COMM", "rccl").lower()
    if v not in ("rccl", "p2p"):
        raise ValueError("AA_COMM must be rccl or p2p, got %r" % v)
    return v


def comm_unique_id():
    buf = ctypes.create_string_buffer(128)
    _check(load_library().aa_comm_get_unique_id(ctypes.cast(buf, _vp)))
    return buf.raw


_uid_serial = [0]


def _publish(path, blob):
    """A rendezvous file other ranks of this launch read: created exclusively with mode 0600 (a file
    somebody else put there first is an error, not an input) and moved into place when complete."""
    tmp = path + ".tmp%d" % os.getpid()
    fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_EXCL, 0o600)
    try:
        os.write(fd, blob)
    finally:
        os.close(fd)
    os.replace(tmp, path)


def _await(path, size, what, rank):
    import time
    deadline = time.time() + 300
    while time.time() < deadline:
        try:
            st = os.stat(path)
            if st.st_size == size and st.st_uid == os.getuid():       # only our own launch's files are trusted
                with open(path, "rb") as fh:
                    return fh.read()
        except OSError:
            pass
        time.sleep(0.02)
    raise RuntimeError("rank %d: timed out waiting for %s (%s)" % (rank, what, path))


def exchange_blobs(rank, world, blob, tag):
    """All-gather of one small byte string per rank through files in the temporary directory of the
    node (single node: the ranks of one launch share MASTER_PORT and the launcher's agent as parent).
    Returns (blobs in rank order, paths)."""
    import tempfile
    _uid_serial[0] += 1
    base = os.path.join(tempfile.gettempdir(), "aa_%s_%s_%d_%d_%d" % (
        tag, os.environ.get("MASTER_PORT", "0"), int(os.environ.get("AA_LAUNCH_ID", os.getppid())), world, _uid_serial[0]))
    paths = ["%s.%d" % (base, r) for r in range(world)]
    _publish(paths[rank], blob)
    return [blob if r == rank else _await(paths[r], len(blob), "rank %d's %s" % (r, tag), rank) for r in range(world)], paths


def exchange_unique_id(rank, world, tag="fit"):
    """Rank 0 draws an RCCL unique id and publishes it through a file in the temporary directory;
    the other ranks of the same launch (same MASTER_PORT, same parent: the launcher's agent -- or the
    same AA_LAUNCH_ID for launchers whose ranks have different parents; single node) wait for it:
    the file is created exclusively with mode 0600, and readers accept only files of their own user.  Every communicator of a process gets its own file (`tag` + a per-process serial,
    which all ranks advance in the same order).  Returns ``(id, path)``."""
    import tempfile
    import time
    _uid_serial[0] += 1
    path = os.path.join(tempfile.gettempdir(), "aa_uid_%s_%d_%d_%s_%d" % (
        os.environ.get("MASTER_PORT", "0"), int(os.environ.get("AA_LAUNCH_ID", os.getppid())), world, tag, _uid_serial[0]))
    if rank == 0:
        uid = comm_unique_id()
        _publish(path, uid)
        return uid, path
    return _await(path, 128, "the RCCL unique id", rank), path


class _Sharded(object):
    """Context manager of a distributed fit's context: closes it after a barrier (a rank must not
    tear its communicator down while another is still inside a collective) and removes the
    rendezvous file."""

    def __init__(self, ctx, uid_path, rank):
        self.ctx, self.uid_path, self.rank = ctx, uid_path, rank

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.ctx.allreduce_host([0.0])
        finally:
            self.ctx.close()
            if self.rank == 0 and self.uid_path:
                try:
                    os.remove(self.uid_path)
                except OSError:
                    pass
        return False


def sharded_context(X, form=FORM_DATA, dtype=None):
    """Context of a distributed fit (see `distributed_env`): this rank's rows of ``X`` on its GPU,
    an RCCL communicator over all ranks, and the global view switched on -- the estimators then
    use it exactly like a single-GPU context."""
    rank, local_rank, world = distributed_env()
    X = np.asarray(X)
    if form != FORM_DATA or X.ndim != 2:
        raise ValueError("a distributed fit needs a data matrix (n_samples x n_features)")
    n = X.shape[0]
    bounds = np.linspace(0, n, world + 1).astype(np.int64)
    lo, hi = int(bounds[rank]), int(bounds[rank + 1])
    if hi <= lo:
        raise ValueError("fewer samples (%d) than ranks (%d)" % (n, world))
    ctx = Context(dtype=dtype, device=device_index())      # LOCAL_RANK, or CONVEX_DIM_RED_DEVICE when set
    try:
        path = None
        if comm_transport() == "p2p":
            ctx.p2p_init(rank, world)
        else:
            uid, path = exchange_unique_id(rank, world)
            ctx.comm_init(uid, rank, world)
        ctx.set_data(X[lo:hi], form=form, n_global=n, row_offset=lo)
        ctx.global_view = True
    except Exception:
        ctx.close()
        raise
    return _Sharded(ctx, path, rank)
