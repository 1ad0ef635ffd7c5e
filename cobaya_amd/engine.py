"""ctypes binding of libmcmc_hip.so (include/mcmc_hip.h) and a thin object wrapper.

The engine has NO CPU fallback: if the shared library is missing, or no gfx950 device is
usable, construction raises `EngineError` -- loudly, by design.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(CSRC, "libmcmc_hip.so")

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)
c_uint64_p = C.POINTER(C.c_uint64)

OK, ERR_ARG, ERR_DEVICE, ERR_NOT_PD, ERR_STATE, ERR_STUCK = 0, -1, -2, -3, -4, -5
ERR_TARGET, ERR_CALLBACK = -6, -7
BESTFIT_QUANTITIES = ("loglike", "logpost")   # mcmc_hip.h: MCMC_HIP_BESTFIT_LOGLIKE / _LOGPOST


class EngineError(RuntimeError):
    """Any failure reported by libmcmc_hip (carries the C error code in `.code`)."""

    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


class NotPositiveDefinite(EngineError):
    pass


class ChainStuck(EngineError):
    pass


class TargetError(EngineError):
    """A function target returned NaN or +inf inside the prior support (MCMC_HIP_ERR_TARGET)."""


# mcmc_hip_loglike_fn: int fn(void* user, int32 n, int32 d, const double* points, double* loglike,
# void* stream) -- the pointers as integers (the wrapper turns them into tensor views)
LOGLIKE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                         C.c_void_p)


class Config(C.Structure):
    _fields_ = [
        ("d", C.c_int32), ("n_walkers", C.c_int32), ("group_size", C.c_int32),
        ("device", C.c_int32), ("seed", C.c_uint64), ("walker_offset", C.c_uint32),
        ("burn_in", C.c_int32), ("temperature", C.c_double), ("proposal_scale", C.c_double),
        ("max_tries", C.c_double), ("emit_capacity", C.c_int32), ("flags", C.c_int32),
    ]


class IncShape(C.Structure):
    """mcmc_hip_inc_shape: the model and ensemble as far as the choice of the incremental kernel
    depends on them (flags are 0 / 1; duo: -1 where it pays, 0 never, 1 wherever it serves)."""
    _fields_ = [(n, C.c_int32) for n in (
        "d", "n_modes", "n_periodic", "n_drag", "n_walkers", "basis_group_size", "any_normal",
        "one_box", "box_lo_is_zero", "has_1d_block", "emit", "duo")]


class IncChoice(C.Structure):
    """mcmc_hip_inc_choice: the kernel family (INC_*) and what that kernel carries."""
    _fields_ = [(n, C.c_int32) for n in (
        "family", "reason", "dq_lo", "carry", "carry_modes", "carry_prior", "carry_periodic",
        "fold", "chunk_steps", "colb", "thins_on_device", "box")]


(INC_NOT_SERVED, INC_STEP, INC_STEP_EMIT, INC_MIX, INC_ANY, INC_DRAG, INC_DUO_MIX,
 INC_DUO_ONE) = range(8)


class ScratchShape(C.Structure):
    """mcmc_hip_scratch_shape: the model and ensemble as far as the choice of the from-scratch step
    kernel depends on them (flags are 0 / 1)."""
    _fields_ = [(n, C.c_int32) for n in (
        "d", "n_modes", "n_walkers", "group_size", "any_normal", "any_periodic", "emit", "emit_thin",
        "unit_t", "own_basis", "blocked", "n_drag", "cps", "cps_f", "has_1d_column")]


class ScratchChoice(C.Structure):
    """mcmc_hip_scratch_answer: the kernel family (SCRATCH_*), its template flags and its launch."""
    _fields_ = [(n, C.c_int32) for n in (
        "family", "reason", "multi", "general", "unit_t", "normp", "unit", "walkers_per_wg", "threads",
        "grid", "lds_bytes", "lds_attr", "v_ld", "slab", "slab_f")]


(SCRATCH_NOT_SERVED, SCRATCH_STEP, SCRATCH_STEP_OWN, SCRATCH_PAIR, SCRATCH_MFMA, SCRATCH_BIG_REG,
 SCRATCH_GENERAL, SCRATCH_DRAG, SCRATCH_GENERAL_DRAG) = range(9)

MOVE_METROPOLIS, MOVE_STRETCH = 0, 1   # mcmc_hip_set_move

# every symbol include/mcmc_hip.h declares: (name, restype, argtypes)
_H = C.c_void_p
SYMBOLS = [
    ("mcmc_hip_version", C.c_char_p, []),
    ("mcmc_hip_last_error", C.c_char_p, [_H]),
    ("mcmc_hip_dim_supported", C.c_int, [C.c_int]),
    ("mcmc_hip_max_dim", C.c_int32, []),
    ("mcmc_hip_incremental_supported", C.c_int, [C.c_int32] * 6),
    ("mcmc_hip_incremental_choice", C.c_int, [C.POINTER(IncShape), C.POINTER(IncChoice)]),
    ("mcmc_hip_scratch_choice", C.c_int, [C.POINTER(ScratchShape), C.POINTER(ScratchChoice)]),
    ("mcmc_hip_create", C.c_int, [C.POINTER(Config), C.POINTER(_H)]),
    ("mcmc_hip_destroy", None, [_H]),
    ("mcmc_hip_set_prior", C.c_int, [_H, c_int32_p, c_double_p, c_double_p, c_int32_p]),
    ("mcmc_hip_set_target_gaussian_mixture", C.c_int,
     [_H, C.c_int32, c_double_p, c_double_p, c_double_p]),
    ("mcmc_hip_set_target_gaussian", C.c_int, [_H, c_double_p, c_double_p, C.c_int32]),
    ("mcmc_hip_set_target_one", C.c_int, [_H]),
    ("mcmc_hip_set_target_function", C.c_int, [_H, LOGLIKE_FN, C.c_void_p]),
    ("mcmc_hip_set_target_functions", C.c_int, [_H, C.c_int32, C.POINTER(LOGLIKE_FN),
                                                C.POINTER(C.c_void_p), c_int32_p, c_int32_p]),
    ("mcmc_hip_get_component_loglikes", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_set_component_loglikes", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_checkpoint_set_ring", C.c_int, [_H, C.c_int32, c_double_p, c_double_p, C.c_int32]),
    ("mcmc_hip_checkpoint_set_accepted", C.c_int, [_H, C.c_int64]),
    ("mcmc_hip_checkpoint_begin", C.c_int, [_H, C.c_int32, C.c_int64, C.c_double,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    ("mcmc_hip_checkpoint_solve", C.c_int, [_H, C.c_double, C.c_double]),
    ("mcmc_hip_checkpoint_fetch", C.c_int, [_H, c_double_p, c_double_p]),
    ("mcmc_hip_checkpoint_request_payload", C.c_int, [_H]),
    ("mcmc_hip_checkpoint_fetch_payload", C.c_int, [_H, c_double_p, C.c_int32]),
    ("mcmc_hip_stream_handle", C.c_uint64, [_H]),
    ("mcmc_hip_drain_samples_pinned", C.c_int, [_H, C.POINTER(c_double_p), c_int64_p]),
    ("mcmc_hip_set_drain_slots", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_set_emit_thin", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_get_thin_carry", C.c_int, [_H, C.POINTER(C.c_int32)]),
    ("mcmc_hip_set_thin_carry", C.c_int, [_H, C.POINTER(C.c_int32)]),
    ("mcmc_hip_set_target_binned_gaussian", C.c_int,
     [_H, C.c_int32, c_int32_p, C.c_int32, c_double_p, c_double_p, c_double_p, C.c_int32,
      c_double_p, c_double_p, c_double_p, C.c_int32]),
    ("mcmc_hip_evaluate_binned", C.c_int,
     [_H, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p]),
    ("mcmc_hip_get_binned_constants", C.c_int, [_H, c_double_p, c_double_p, c_double_p]),
    ("mcmc_hip_binned_kernel_times", C.c_int, [_H, c_double_p, c_int64_p, C.c_int32]),
    ("mcmc_hip_set_blocking", C.c_int, [_H, C.c_int32, c_int32_p, c_int32_p, c_int32_p,
                                        C.c_int32, C.c_int32]),
    ("mcmc_hip_cycle_length", C.c_int, [_H]),
    ("mcmc_hip_set_proposal_cov", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_get_proposal_cov", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_get_proposal_transform", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_evaluate", C.c_int, [_H, C.c_int32, c_double_p, c_double_p, c_double_p,
                                    c_double_p]),
    ("mcmc_hip_set_state", C.c_int, [_H, c_double_p, c_int32_p]),
    ("mcmc_hip_get_state", C.c_int, [_H, c_double_p, c_double_p, c_double_p, c_double_p,
                                     c_int32_p]),
    ("mcmc_hip_get_full_state", C.c_int, [_H, c_double_p, c_double_p, c_double_p, c_double_p,
                                          c_int32_p, c_int32_p, c_int32_p, c_int64_p,
                                          C.POINTER(C.c_uint64)]),
    ("mcmc_hip_set_full_state", C.c_int, [_H, c_double_p, c_double_p, c_double_p, c_double_p,
                                          c_int32_p, c_int32_p, c_int32_p, c_int64_p,
                                          C.c_uint64]),
    ("mcmc_hip_step", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_set_move", C.c_int, [_H, C.c_int32, C.c_double]),
    ("mcmc_hip_set_moves", C.c_int, [_H, C.c_int32, c_int32_p, c_double_p, c_double_p, c_double_p]),
    ("mcmc_hip_sync", C.c_int, [_H]),
    ("mcmc_hip_get_counters", C.c_int, [_H, c_int64_p]),
    ("mcmc_hip_drain_samples", C.c_int, [_H, c_double_p, C.c_int64, c_int64_p]),
    ("mcmc_hip_get_derived_constants", C.c_int, [_H, c_double_p, c_double_p, c_double_p,
                                                 c_double_p, c_double_p]),
    ("mcmc_hip_set_moment_shift", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_accumulate_moments", C.c_int, [_H]),
    ("mcmc_hip_read_moments", C.c_int, [_H, c_int64_p, c_double_p, c_double_p, C.c_int32]),
    ("mcmc_hip_set_moments", C.c_int, [_H, C.c_int64, c_double_p, c_double_p]),
    ("mcmc_hip_request_moments", C.c_int, [_H]),
    ("mcmc_hip_fetch_moments", C.c_int, [_H, c_int64_p, c_double_p, c_double_p, c_int64_p]),
    ("mcmc_hip_marginals_configure", C.c_int, [_H, C.c_int32, c_int32_p, C.c_int32, C.c_int32,
                                               c_int32_p, C.c_int32, c_double_p, c_double_p]),
    ("mcmc_hip_marginals_accumulate", C.c_int, [_H]),
    ("mcmc_hip_marginals_request", C.c_int, [_H]),
    ("mcmc_hip_marginals_fetch", C.c_int, [_H, c_uint64_p, C.c_int64, c_int64_p]),
    ("mcmc_hip_marginals_set", C.c_int, [_H, c_uint64_p, C.c_int64, C.c_int64]),
    ("mcmc_hip_marginals_layout", C.c_int, [_H, c_int64_p, c_int32_p, c_int32_p, c_int32_p,
                                            c_int32_p, c_int64_p]),
    ("mcmc_hip_autocorr_configure", C.c_int, [_H, C.c_int32, c_int32_p, C.c_int32]),
    ("mcmc_hip_autocorr_accumulate", C.c_int, [_H]),
    ("mcmc_hip_autocorr_request", C.c_int, [_H]),
    ("mcmc_hip_autocorr_fetch", C.c_int, [_H, c_double_p, C.c_int64, c_int64_p]),
    ("mcmc_hip_autocorr_set", C.c_int, [_H, c_double_p, C.c_int64, c_int64_p]),
    ("mcmc_hip_autocorr_reset", C.c_int, [_H]),
    ("mcmc_hip_autocorr_layout", C.c_int, [_H, c_int32_p, c_int32_p, c_int64_p, c_int32_p]),
    ("mcmc_hip_bestfit_configure", C.c_int, [_H, C.c_int32, c_int32_p, C.c_int32, c_double_p, c_double_p,
                                             C.c_int32]),
    ("mcmc_hip_bestfit_accumulate", C.c_int, [_H]),
    ("mcmc_hip_bestfit_request", C.c_int, [_H]),
    ("mcmc_hip_bestfit_fetch", C.c_int, [_H, c_uint64_p, C.c_int64, c_uint64_p, C.c_int64, c_int64_p]),
    ("mcmc_hip_bestfit_set", C.c_int, [_H, c_uint64_p, C.c_int64, c_uint64_p, C.c_int64, C.c_int64]),
    ("mcmc_hip_evidence_configure", C.c_int, [_H, C.c_int32, c_double_p]),
    ("mcmc_hip_evidence_set_ellipsoid", C.c_int, [_H, c_double_p, c_double_p]),
    ("mcmc_hip_evidence_accumulate", C.c_int, [_H]),
    ("mcmc_hip_evidence_request", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_evidence_fetch", C.c_int, [_H, c_double_p, c_uint64_p, C.c_int64, c_uint64_p, c_int64_p,
                                          c_double_p, c_double_p, C.c_int64, c_int32_p, c_int32_p]),
    ("mcmc_hip_evidence_set", C.c_int, [_H, c_double_p, c_uint64_p, C.c_int64, C.c_uint64, C.c_int64,
                                        c_double_p, c_double_p, C.c_int64]),
    ("mcmc_hip_evidence_layout", C.c_int, [_H, c_int32_p, c_int32_p, c_int32_p, c_int64_p, c_int32_p,
                                           c_int32_p, c_int64_p]),
    ("mcmc_hip_bestfit_layout", C.c_int, [_H, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int64_p,
                                          c_int64_p]),
    ("mcmc_hip_importance_configure", C.c_int, [_H, C.c_int32, c_int32_p]),
    ("mcmc_hip_importance_set_group_size", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_importance_layout", C.c_int, [_H, c_int32_p, c_int32_p, c_int64_p, c_int64_p, c_int32_p, c_int64_p,
                                             C.POINTER(C.c_uint64)]),
    ("mcmc_hip_importance_accumulate", C.c_int, [_H, C.c_uint64]),
    ("mcmc_hip_importance_request", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_importance_fetch", C.c_int, [_H, c_double_p, C.c_int64, c_uint64_p, C.c_int64, c_uint64_p,
                                            c_double_p, c_int64_p]),
    ("mcmc_hip_importance_set", C.c_int, [_H, c_double_p, C.c_int64, c_uint64_p, C.c_int64, c_uint64_p,
                                          c_double_p, C.c_int64]),
    ("mcmc_hip_importance_hist_configure", C.c_int, [_H, c_int32_p]),
    ("mcmc_hip_importance_hist_layout", C.c_int, [_H, c_int32_p, c_int32_p, c_int64_p, c_int64_p]),
    ("mcmc_hip_importance_hist_fetch", C.c_int, [_H, c_uint64_p, c_uint64_p, C.c_int64, c_uint64_p, c_int64_p]),
    ("mcmc_hip_importance_hist_set", C.c_int, [_H, c_uint64_p, c_uint64_p, C.c_int64, c_uint64_p]),
    ("mcmc_hip_derived_configure", C.c_int, [_H, C.c_int32, C.c_int32, c_int32_p, c_double_p]),
    ("mcmc_hip_derived_set_group_size", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_derived_layout", C.c_int, [_H, c_int32_p, c_int32_p, c_int32_p, c_int64_p]),
    ("mcmc_hip_derived_buffers", C.c_int, [_H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("mcmc_hip_derived_set_values", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_derived_get_values", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_derived_accumulate", C.c_int, [_H]),
    ("mcmc_hip_derived_request", C.c_int, [_H]),
    ("mcmc_hip_derived_fetch", C.c_int, [_H, c_uint64_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                         c_double_p, c_uint64_p, c_double_p, c_double_p, c_int64_p]),
    ("mcmc_hip_derived_set", C.c_int, [_H, C.c_uint64, c_double_p, c_double_p, c_double_p, c_double_p,
                                       c_double_p, c_uint64_p, c_double_p, c_double_p, C.c_int64]),
    ("mcmc_hip_gelman_rubin", C.c_int, [C.c_int32, C.c_double, C.c_double, c_double_p,
                                        c_double_p, c_double_p, c_double_p, c_double_p]),
    ("mcmc_hip_enable_timing", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_last_step_kernel", C.c_char_p, [_H]),
    ("mcmc_hip_get_whitened", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_set_whitened", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_incremental_carries_modes", C.c_int, [_H]),
    ("mcmc_hip_incremental_carries_periodic", C.c_int, [_H]),
    ("mcmc_hip_accept_estimate_error", C.c_int, [c_double_p, C.POINTER(C.c_uint32)]),
    ("mcmc_hip_math_probe", C.c_int, [C.c_int32, c_uint64_p, C.c_uint64, C.c_uint64, C.c_int64, c_uint64_p]),
    ("mcmc_hip_get_mode_logdensities", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_set_mode_logdensities", C.c_int, [_H, c_double_p]),
    ("mcmc_hip_kernel_times", C.c_int, [_H, c_double_p, c_int64_p, C.c_int32]),
    ("mcmc_hip_bounds_configure", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_bounds_snapshot", C.c_int, [_H, C.c_int32]),
    ("mcmc_hip_bounds_statistics", C.c_int, [_H, C.c_int32, c_int32_p, C.c_double, c_double_p,
                                            c_double_p]),
    ("mcmc_hip_bounds_get_slot", C.c_int, [_H, C.c_int32, c_double_p]),
    ("mcmc_hip_bounds_set_slot", C.c_int, [_H, C.c_int32, c_double_p]),
    ("mcmc_hip_comm_version", C.c_char_p, []),
    ("mcmc_hip_comm_last_error", C.c_char_p, [_H]),
    ("mcmc_hip_comm_unique_id", C.c_int, [C.POINTER(C.c_uint8)]),
    ("mcmc_hip_comm_create", C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(_H)]),
    ("mcmc_hip_comm_destroy", None, [_H]),
    ("mcmc_hip_comm_rank", C.c_int, [_H]),
    ("mcmc_hip_comm_size", C.c_int, [_H]),
    ("mcmc_hip_comm_allreduce", C.c_int, [_H, c_double_p, C.c_int64, C.c_int32]),
    ("mcmc_hip_comm_allreduce_device", C.c_int, [_H, C.c_uint64, C.c_int64, C.c_int32, C.c_uint64]),
    ("mcmc_hip_comm_time_allreduce", C.c_int, [_H, C.c_int64, C.c_int32, c_double_p]),
    ("mcmc_hip_set_comm", C.c_int, [_H, _H]),
]

_lib = None


def load_library(path: str | None = None):
    """dlopen libmcmc_hip.so and bind every declared symbol (raises if anything is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # MCMC_HIP_LIB (developer switch): an experiment build of the same ABI (tools/exp_*.sh)
    path = path or os.environ.get("MCMC_HIP_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise EngineError(ERR_DEVICE,
                          f"{path} not found: build it with `python -m cobaya_amd.build` "
                          "(hipcc, gfx950). mcmc_hip has no CPU fallback.")
    lib = C.CDLL(path)
    for name, restype, argtypes in SYMBOLS:
        try:
            fn = getattr(lib, name)  # AttributeError if the library does not export it
        except AttributeError:
            # developer A/B runs against an OLDER build of the library (MCMC_HIP_LIB=... with
            # MCMC_HIP_LIB_COMPAT=1, tools/gpu.sh ab): an entry point it predates answers "no" --
            # 0 for the predicates (`*_supported`, `*carries_*`), MCMC_HIP_ERR_ARG for every
            # setter and getter: a missing mcmc_hip_set_emit_thin must not look like success
            # (the sampler then skipped host thinning and rows came out un-thinned)
            if not (os.environ.get("MCMC_HIP_LIB_COMPAT") and os.environ.get("MCMC_HIP_LIB")):
                raise
            predicate = "carries_" in name or name.endswith("_supported")
            answer = 0 if predicate or restype is not C.c_int else ERR_ARG
            setattr(lib, name, C.CFUNCTYPE(restype, *argtypes)(lambda *a, _r=answer: _r))
            continue
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _ip(a):
    return a.ctypes.data_as(c_int32_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected array of shape {tuple(shape)}, got {a.shape}")
    return a


def max_dim():
    """The largest number of sampled parameters the library serves (mcmc_hip_max_dim)."""
    return int(load_library().mcmc_hip_max_dim())


def incremental_supported(d, n_modes, n_periodic, n_drag, n_walkers, basis_group_size):
    """Does incremental evaluation (O(d) steps on carried whitened residuals) serve this model
    shape?  (mcmc_hip_incremental_supported: a pure function of the library, no device.)"""
    return bool(load_library().mcmc_hip_incremental_supported(
        int(d), int(n_modes), int(n_periodic), int(n_drag), int(n_walkers), int(basis_group_size)))


def incremental_choice(d, n_modes, n_periodic=0, n_drag=0, n_walkers=65536, basis_group_size=256,
                       any_normal=False, one_box=False, box_lo_is_zero=False, has_1d_block=False,
                       emit=False, duo=-1):
    """Which incremental step kernel serves this shape and what it carries, as a dict of the
    fields of mcmc_hip_inc_choice (mcmc_hip_incremental_choice: the library's one rule, a pure
    function -- no device).  family == INC_NOT_SERVED: `reason` says why."""
    shape = IncShape(int(d), int(n_modes), int(n_periodic), int(n_drag), int(n_walkers),
                     int(basis_group_size), int(any_normal), int(one_box), int(box_lo_is_zero),
                     int(has_1d_block), int(emit), int(duo))
    out = IncChoice()
    rc = load_library().mcmc_hip_incremental_choice(C.byref(shape), C.byref(out))
    if rc != OK:
        raise EngineError(rc, "mcmc_hip_incremental_choice is not served by this library")
    return {n: int(getattr(out, n)) for n, _ in IncChoice._fields_}


def scratch_choice(d, n_modes=1, n_walkers=65536, group_size=256, any_normal=False, any_periodic=False,
                   emit=False, emit_thin=False, unit_t=True, own_basis=False, blocked=False, n_drag=0,
                   cps=0, cps_f=0, has_1d_column=False):
    """Which from-scratch step kernel serves this shape and how it is launched, as a dict of the
    fields of mcmc_hip_scratch_answer (mcmc_hip_scratch_choice: the library's one rule, a pure
    function -- no device).  family == SCRATCH_NOT_SERVED: `reason` says why."""
    shape = ScratchShape(int(d), int(n_modes), int(n_walkers), int(group_size), int(any_normal),
                         int(any_periodic), int(emit), int(emit_thin), int(unit_t), int(own_basis),
                         int(blocked), int(n_drag), int(cps), int(cps_f), int(has_1d_column))
    out = ScratchChoice()
    rc = load_library().mcmc_hip_scratch_choice(C.byref(shape), C.byref(out))
    if rc != OK:
        raise EngineError(rc, "mcmc_hip_scratch_choice is not served by this library")
    return {n: int(getattr(out, n)) for n, _ in ScratchChoice._fields_}


def gelman_rubin(n_chains, sum_N, sum_Ncov, sum_mean, sum_mm):
    """R-1 of means and the N-weighted mean of covariances from reduced sufficient
    statistics (mcmc.py:856-889).  Raises NotPositiveDefinite where the reference skips the
    update on LinAlgError (mcmc.py:870-887)."""
    lib = load_library()
    sum_mean = _f64(sum_mean)
    d = len(sum_mean)
    sum_Ncov, sum_mm = _f64(sum_Ncov, (d, d)), _f64(sum_mm, (d, d))
    R = C.c_double()
    W = np.empty((d, d))
    rc = lib.mcmc_hip_gelman_rubin(d, float(n_chains), float(sum_N), _dp(sum_Ncov),
                                   _dp(sum_mean), _dp(sum_mm), C.byref(R), _dp(W))
    if rc == ERR_NOT_PD:
        raise NotPositiveDefinite(rc, "Negative covariance eigenvectors / not enough "
                                      "information in the samples to compute R-1")
    if rc:
        raise EngineError(rc, "gelman_rubin: invalid arguments")
    return R.value, W


COMM_ID_BYTES = 128


class Communicator:
    """The walker shards' communicator inside libmcmc_hip.so (RCCL over xGMI; one handle of
    `mcmc_hip_comm_*`).  Creation is collective over all ranks."""

    _OPS = {"sum": 0, "max": 1}

    @staticmethod
    def unique_id() -> bytes:
        """Rank 0: the 128-byte id every rank's constructor needs (ncclGetUniqueId)."""
        lib = load_library()
        ident = (C.c_uint8 * COMM_ID_BYTES)()
        if lib.mcmc_hip_comm_unique_id(ident):
            raise EngineError(ERR_DEVICE, lib.mcmc_hip_comm_last_error(None).decode())
        return bytes(ident)

    def __init__(self, ident: bytes, rank: int, size: int, device: int):
        self._lib = load_library()
        if len(ident) != COMM_ID_BYTES:
            raise EngineError(ERR_ARG, f"the communicator id has {COMM_ID_BYTES} bytes")
        self._h = _H()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(ident)
        rc = self._lib.mcmc_hip_comm_create(buf, int(rank), int(size), int(device), C.byref(self._h))
        if rc:
            self._h = _H()
            raise EngineError(rc, "mcmc_hip_comm_create failed: "
                              + self._lib.mcmc_hip_comm_last_error(None).decode())
        self.rank, self.size, self.device = int(rank), int(size), int(device)
        self.version = self._lib.mcmc_hip_comm_version().decode()

    def _check(self, rc):
        if rc:
            raise EngineError(rc, self._lib.mcmc_hip_comm_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    def allreduce(self, buf: np.ndarray, op="sum") -> np.ndarray:
        """In place over ranks, a float64 HOST buffer (staged through pinned memory; synchronous)."""
        flat = np.ascontiguousarray(buf, dtype=np.float64).reshape(-1)
        self._check(self._lib.mcmc_hip_comm_allreduce(self._h, _dp(flat), flat.size, self._OPS[op]))
        buf[...] = flat.reshape(buf.shape)
        return buf

    def allreduce_device(self, ptr: int, n: int, op="sum", stream: int = 0):
        """In place, n float64 at a device pointer, queued in order on `stream` (0: its own)."""
        self._check(self._lib.mcmc_hip_comm_allreduce_device(self._h, int(ptr), int(n), self._OPS[op],
                                                             int(stream)))

    def time_allreduce(self, n: int, reps: int = 20) -> float:
        """HIP-event microseconds per in-stream all-reduce of n float64 (collective)."""
        us = C.c_double()
        self._check(self._lib.mcmc_hip_comm_time_allreduce(self._h, int(n), int(reps), C.byref(us)))
        return us.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mcmc_hip_comm_destroy(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One walker ensemble on one MI355X (one handle of the C ABI)."""

    @staticmethod
    def max_dim():
        """The largest number of sampled parameters the library serves (mcmc_hip_max_dim)."""
        return max_dim()

    def __init__(self, d, n_walkers, group_size=64, device=0, seed=0, walker_offset=0,
                 burn_in=0, temperature=1.0, proposal_scale=2.4, max_tries=None,
                 emit_capacity=0, shared_basis=True, incremental=False, basis_group_size=None):
        self._lib = load_library()
        self.incremental = bool(incremental)
        # walkers sharing one Haar basis: group_size * 2**m (incremental mode only)
        bgs = int(basis_group_size or group_size)
        m = (bgs // int(group_size)).bit_length() - 1
        if bgs != int(group_size) << m:
            raise EngineError(ERR_ARG, "basis_group_size must be group_size times a power of two")
        self.basis_group_size = bgs
        self._h = _H()
        self.d, self.W, self.group_size = int(d), int(n_walkers), int(group_size)
        self.G = self.W // self.group_size if self.group_size else 0
        self.K = None
        self.walker_offset = int(walker_offset)
        cfg = Config(d=d, n_walkers=n_walkers, group_size=group_size, device=device,
                     seed=int(seed) & (2 ** 64 - 1), walker_offset=walker_offset,
                     burn_in=int(burn_in), temperature=float(temperature),
                     proposal_scale=float(proposal_scale),
                     max_tries=float(max_tries if max_tries is not None else 40 * d),
                     emit_capacity=int(emit_capacity), flags=(0 if shared_basis else 1) | (2 if incremental else 0) | (m << 8))
        self.cfg = cfg
        rc = self._lib.mcmc_hip_create(C.byref(cfg), C.byref(self._h))
        if rc:
            msg = self._lib.mcmc_hip_last_error(None).decode()
            self._h = _H()
            raise EngineError(rc, f"mcmc_hip_create failed: {msg}")

    # -- plumbing
    def _check(self, rc):
        if rc == OK:
            return
        msg = self._lib.mcmc_hip_last_error(self._h).decode()
        cls = {ERR_NOT_PD: NotPositiveDefinite, ERR_STUCK: ChainStuck,
               ERR_TARGET: TargetError}.get(rc, EngineError)
        if rc == ERR_CALLBACK and self._fn_exc is not None:
            # an exception cannot cross the C callback: the wrapper kept it, and it is the cause
            exc, self._fn_exc = self._fn_exc, None
            if not isinstance(exc, Exception):   # KeyboardInterrupt, SystemExit: not ours to wrap
                raise exc
            raise EngineError(rc, f"{msg}: the target function raised "
                                  f"{type(exc).__name__}: {exc}") from exc
        raise cls(rc, msg)

    _fn_exc = None
    _fn_callback = None
    n_derived = n_derived_cross = 0    # (configure_derived)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mcmc_hip_destroy(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- problem
    def set_prior(self, kinds, a, b, periodic=None):
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        a, b = _f64(a, (self.d,)), _f64(b, (self.d,))
        per = (np.zeros(self.d, np.int32) if periodic is None
               else np.ascontiguousarray(periodic, dtype=np.int32))
        self._check(self._lib.mcmc_hip_set_prior(self._h, _ip(kinds), _dp(a), _dp(b), _ip(per)))

    def set_target_gaussian_mixture(self, means, covs, weights=None):
        means = _f64(np.atleast_2d(means))
        K = len(means)
        covs = _f64(covs).reshape(K, self.d, self.d)
        w = None if weights is None else _f64(np.atleast_1d(weights), (K,))
        self._check(self._lib.mcmc_hip_set_target_gaussian_mixture(
            self._h, K, _dp(means), _dp(covs), _dp(w) if w is not None else None))
        self.K = K

    def set_target_gaussian(self, mean, cov, normalized=True):
        mean, cov = _f64(mean, (self.d,)), _f64(cov, (self.d, self.d))
        self._check(self._lib.mcmc_hip_set_target_gaussian(self._h, _dp(mean), _dp(cov),
                                                           int(bool(normalized))))
        self.K = 1

    def set_target_binned_gaussian(self, target, emulator, calib_index):
        """`target`: a `cobaya_amd.pliklite.BinnedGaussian` (what PlanckPlikLite.init_params
        leaves on the likelihood, planck_pliklite.py:32-141); `emulator`: a `LinearClEmulator`
        for the d - 1 other sampled parameters; `calib_index`: position of the calibration
        parameter among the sampled ones."""
        bins = np.ascontiguousarray(target.bin_table(), dtype=np.int32)
        n = len(bins)
        w = _f64(target.weights, (target.lmax + 1,))
        X, cov = _f64(target.X_data, (n,)), _f64(target.cov, (n, n))
        th = _f64(emulator.theta0, (self.d - 1,))
        D0 = _f64(emulator.D0, (3, target.lmax + 1))
        J = _f64(emulator.J, (3, target.lmax + 1, self.d - 1))
        self._check(self._lib.mcmc_hip_set_target_binned_gaussian(
            self._h, n, _ip(bins), int(target.lmax), _dp(w), _dp(X), _dp(cov), self.d - 1,
            _dp(th), _dp(D0), _dp(J), int(calib_index)))
        self.K = 0
        self.n_bins = n

    def binned_constants(self):
        n = self.n_bins
        Linv, Bc0, BJ = np.empty((n, n)), np.empty(n), np.empty((n, self.d - 1))
        self._check(self._lib.mcmc_hip_get_binned_constants(self._h, _dp(Linv), _dp(Bc0), _dp(BJ)))
        return {"Linv": Linv, "Bc0": Bc0, "BJ": BJ}

    def evaluate_binned(self, L0, cl, A):
        """chi2[n] = get_chi_squared(L0, cl[k, 0], cl[k, 1], cl[k, 2], A[k]) on the device."""
        cl = _f64(cl)
        n, three, n_ell = cl.shape
        assert three == 3
        A = _f64(np.broadcast_to(np.asarray(A, dtype=np.float64), (n,)))
        out = np.empty(n)
        self._check(self._lib.mcmc_hip_evaluate_binned(self._h, n, int(L0), n_ell, _dp(cl), _dp(A),
                                                       _dp(out)))
        return out

    def binned_kernel_times(self, reset=False):
        ms, n = np.zeros(3), np.zeros(3, np.int64)
        self._check(self._lib.mcmc_hip_binned_kernel_times(self._h, _dp(ms), n.ctypes.data_as(c_int64_p),
                                                           int(bool(reset))))
        return {"walker_ms": ms[0], "residual_ms": ms[1], "chi2_ms": ms[2],
                "launches": [int(v) for v in n]}

    def set_target_one(self):
        self._check(self._lib.mcmc_hip_set_target_one(self._h))
        self.K = 0

    def set_target_function(self, fn, pass_out=False):
        """Target kind `function` (mcmc_hip_set_target_function): the log-likelihood of a point is
        what `fn` returns for it.

        `fn(points)` receives a torch.float64 tensor (n, d) on the engine's device -- a VIEW of
        the engine's buffer of trial points, sampled parameters in sampled order -- and returns
        (n,) float64 log-likelihoods on that device.  It is called once per step with the trials
        of all walkers, under the engine's stream (`torch.cuda.ExternalStream`): its operations
        are stream-ordered with the step kernels and nothing synchronises with the host.

        Rows outside the prior support are included; what it returns for them is ignored (NaN is
        allowed there).  Inside the support -inf rejects the trial; NaN or +inf raise
        `TargetError` at the next `sync` / `fetch_moments`.  An exception inside `fn` is re-raised
        as the cause of the `EngineError` of the `step` / `evaluate` that called it; the engine
        stays usable.

        `pass_out=True`: `fn` is called as `fn(points, out)` with the engine's (n,) result buffer
        as a second argument; a result returned from there is not copied.

        `import torch` before the first Engine is created: PyTorch brings its own copy of the HIP
        runtime, which the process must load first."""
        if not callable(fn):
            raise EngineError(ERR_ARG, f"set_target_function needs a callable, got {fn!r}")
        stream, make = self._function_callbacks()
        cb = LOGLIKE_FN(make(fn, pass_out))
        self._check(self._lib.mcmc_hip_set_target_function(self._h, cb, None))
        self._fn_callback = (cb, fn, stream)   # alive as long as the engine
        self.K = 0
        self.n_functions = 0

    def _function_callbacks(self):
        """(the engine's stream as PyTorch sees it, make(fn, pass_out) -> the C callback's body)."""
        import torch   # (only function targets need it)
        dev = torch.device("cuda", int(self.cfg.device))
        try:
            stream = torch.cuda.ExternalStream(self.stream_handle(), device=dev)
        except RuntimeError as e:
            # PyTorch ships its own copy of the HIP runtime: loaded after libmcmc_hip.so has bound
            # to the system's, the process holds two runtimes and PyTorch's finds no device
            raise EngineError(ERR_DEVICE,
                              f"PyTorch cannot use device {dev} in this process ({e}): `import torch` "
                              "before the first Engine is created (before libmcmc_hip.so is loaded), so "
                              "that both use one HIP runtime") from e
        views = {}

        class _View:   # __cuda_array_interface__ of n float64 at a device pointer: no copy
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f8", "data": (ptr, False),
                                                 "version": 2, "strides": None}

        def view(ptr, shape):
            key = (ptr, shape)
            t = views.get(key)
            if t is None:
                if len(views) > 64:
                    views.clear()
                t = views[key] = torch.as_tensor(_View(ptr, shape), device=dev)
            return t

        def make(fn, pass_out):
            pass_out = bool(pass_out)

            def callback(_user, n, d, points, loglike, _stream):
                try:
                    with torch.cuda.stream(stream):
                        out_buf = view(loglike, (n,))
                        pts = view(points, (n, d))
                        out = fn(pts, out_buf) if pass_out else fn(pts)
                        if not isinstance(out, torch.Tensor):
                            raise TypeError("the target function must return a torch.Tensor, got "
                                            f"{type(out).__name__}")
                        if tuple(out.shape) != (n,):
                            raise ValueError(f"the target function must return shape ({n},), got shape "
                                             f"{tuple(out.shape)}")
                        if out.dtype != torch.float64:
                            raise TypeError("the target function must return dtype torch.float64, got "
                                            f"dtype {out.dtype}")
                        if out.device != dev:
                            raise ValueError(f"the target function must return a tensor on device {dev}, "
                                             f"got device {out.device}")
                        if out.data_ptr() != loglike or not out.is_contiguous():
                            out_buf.copy_(out)
                    return 0
                except BaseException as e:   # (cannot cross ctypes: kept for _check, which re-raises
                    # a KeyboardInterrupt / SystemExit as it is)
                    self._fn_exc = e
                    return 1
            return callback

        return stream, make

    n_functions = 0    # (set_target_functions)

    def set_target_functions(self, fns, inputs, pass_out=False):
        """Target kind `function` with several functions over parameter blocks
        (mcmc_hip_set_target_functions): the log-likelihood is the sum of 1..8 batched device
        functions.  `inputs[c]`: the sampler indices function c reads; `fns[c](points)` receives them
        as a torch.float64 tensor (n, len(inputs[c])) in that order and returns (n,) float64, under
        the conventions of `set_target_function`.  The subsets may overlap; every sampled parameter
        feeds at least one function.  Accepts `set_blocking` (no dragging): at a slot of block b only
        the functions with an input in a block >= b are called, the others keep their carried value
        (`get_full_state()["ll_c"]`)."""
        fns, inputs = list(fns), [[int(i) for i in idx] for idx in inputs]
        if len(fns) != len(inputs) or not all(callable(f) for f in fns):
            raise EngineError(ERR_ARG, "set_target_functions needs one list of inputs per callable")
        stream, make = self._function_callbacks()
        cbs = [LOGLIKE_FN(make(f, pass_out)) for f in fns]
        arr = (LOGLIKE_FN * len(cbs))(*cbs)
        n_in = np.array([len(i) for i in inputs], dtype=np.int32)
        flat = np.array([i for idx in inputs for i in idx], dtype=np.int32)
        self._check(self._lib.mcmc_hip_set_target_functions(self._h, len(cbs), arr, None, _ip(n_in), _ip(flat)))
        self._fn_callback = (cbs, arr, fns, stream)   # alive as long as the engine
        self.K = 0
        self.n_functions = len(cbs)

    def get_component_loglikes(self):
        """ll_c[n_functions][n_walkers]: the carried per-function log-likelihoods of the state."""
        out = np.empty((self.n_functions, self.W))
        self._check(self._lib.mcmc_hip_get_component_loglikes(self._h, _dp(out)))
        return out

    def set_component_loglikes(self, ll_c):
        self._check(self._lib.mcmc_hip_set_component_loglikes(self._h, _dp(_f64(ll_c, (self.n_functions, self.W)))))

    def derived_constants(self):
        d, K = self.d, max(self.K or 0, 0)
        u = C.c_double()
        mls = np.empty(d)
        Linv, cn, w = np.empty((max(K, 1), d, d)), np.empty(max(K, 1)), np.empty(max(K, 1))
        self._check(self._lib.mcmc_hip_get_derived_constants(
            self._h, C.byref(u), _dp(mls), _dp(Linv) if K else None, _dp(cn) if K else None,
            _dp(w) if K else None))
        return {"uniform_logp": u.value, "mls": mls, "Linv": Linv[:K], "cnorm": cn[:K],
                "weight": w[:K]}

    def set_blocking(self, blocks, oversampling=None, drag_last_slow=-1, drag_steps=0):
        """Parameter blocks (lists of sampler indices, slow -> fast) with their oversampling
        factors (proposal.py:96-196); drag_last_slow >= 0 selects the dragging step."""
        sizes = np.array([len(b) for b in blocks], dtype=np.int32)
        over = np.array(oversampling if oversampling is not None else [1] * len(blocks),
                        dtype=np.int32)
        i_of_j = np.array([i for b in blocks for i in b], dtype=np.int32)
        if len(i_of_j) != self.d or len(over) != len(sizes):
            raise EngineError(ERR_ARG, "The blocks do not contain all the parameter indices.")
        self._check(self._lib.mcmc_hip_set_blocking(
            self._h, len(sizes), _ip(sizes), _ip(over), _ip(i_of_j), int(drag_last_slow),
            int(drag_steps)))

    def cycle_length(self):
        return int(self._lib.mcmc_hip_cycle_length(self._h))

    def set_proposal_cov(self, cov):
        cov = _f64(cov, (self.d, self.d))
        self._check(self._lib.mcmc_hip_set_proposal_cov(self._h, _dp(cov)))

    def get_proposal_cov(self):
        out = np.empty((self.d, self.d))
        self._check(self._lib.mcmc_hip_get_proposal_cov(self._h, _dp(out)))
        return out

    def get_proposal_transform(self):
        out = np.empty((self.d, self.d))
        self._check(self._lib.mcmc_hip_get_proposal_transform(self._h, _dp(out)))
        return out

    # -- evaluation / state
    def evaluate(self, x, derived=False):
        x = _f64(np.atleast_2d(x))
        n = len(x)
        lp, ll = np.empty(n), np.empty(n)
        der = np.empty((n, max(self.K or 0, 1) * self.d)) if derived else None
        self._check(self._lib.mcmc_hip_evaluate(self._h, n, _dp(x), _dp(lp), _dp(ll),
                                                _dp(der) if derived else None))
        return (lp, ll, der) if derived else (lp, ll)

    def set_state(self, x):
        x = _f64(x, (self.W, self.d))
        bad = C.c_int32()
        self._check(self._lib.mcmc_hip_set_state(self._h, _dp(x), C.byref(bad)))

    def get_state(self):
        x = np.empty((self.W, self.d))
        lpost, lpri, llik = np.empty(self.W), np.empty(self.W), np.empty(self.W)
        wt = np.empty(self.W, np.int32)
        self._check(self._lib.mcmc_hip_get_state(self._h, _dp(x), _dp(lpost), _dp(lpri),
                                                 _dp(llik), _ip(wt)))
        return {"x": x, "logpost": lpost, "logprior": lpri, "loglike": llik, "weight": wt}

    def get_full_state(self):
        """Everything needed to resume bit-identically (see mcmc_hip_get_full_state)."""
        W = self.W
        out = {"x": np.empty((W, self.d)), "logpost": np.empty(W), "logprior": np.empty(W),
               "loglike": np.empty(W), "weight": np.empty(W, np.int32),
               "prior_rej": np.empty(W, np.int32), "burn_left": np.empty(W, np.int32),
               "n_accept": np.empty(W, np.int64)}
        step = C.c_uint64()
        self._check(self._lib.mcmc_hip_get_full_state(
            self._h, _dp(out["x"]), _dp(out["logpost"]), _dp(out["logprior"]),
            _dp(out["loglike"]), _ip(out["weight"]), _ip(out["prior_rej"]),
            _ip(out["burn_left"]), out["n_accept"].ctypes.data_as(c_int64_p), C.byref(step)))
        out["step"] = np.uint64(step.value)
        if self.incremental:   # the carried whitened residual is part of the state
            out["y"] = np.empty((W, max(self.K or 1, 1) * self.d))
            self._check(self._lib.mcmc_hip_get_whitened(self._h, _dp(out["y"])))
            if self.carries_modes():
                # the carried log-density of every mode (mixtures on step_inc_mix_kernel); absent
                # until a step has formed them (they are then re-anchored on y by the next one)
                am = np.empty((W, self.K))
                if self._lib.mcmc_hip_get_mode_logdensities(self._h, _dp(am)) == 0:
                    out["amode"] = am
        if self.emit_thin > 1:   # thinned emission on the device: the per-walker remainders
            out["thin_carry"] = self.get_thin_carry()
        if self.n_functions:     # several functions: the carried per-function values
            out["ll_c"] = self.get_component_loglikes()
        return out

    def set_full_state(self, st):
        W = self.W
        x = _f64(st["x"], (W, self.d))
        f = {k: _f64(st[k], (W,)) for k in ("logpost", "logprior", "loglike")}
        i = {k: np.ascontiguousarray(st[k], dtype=np.int32) for k in
             ("weight", "prior_rej", "burn_left")}
        na = np.ascontiguousarray(st["n_accept"], dtype=np.int64)
        self._check(self._lib.mcmc_hip_set_full_state(
            self._h, _dp(x), _dp(f["logpost"]), _dp(f["logprior"]), _dp(f["loglike"]),
            _ip(i["weight"]), _ip(i["prior_rej"]), _ip(i["burn_left"]),
            na.ctypes.data_as(c_int64_p), int(st["step"])))
        if self.incremental and "y" in st:
            y = _f64(st["y"], (W, max(self.K or 1, 1) * self.d))
            self._check(self._lib.mcmc_hip_set_whitened(self._h, _dp(y)))
            if "amode" in st and self.carries_modes():
                am = _f64(st["amode"], (W, self.K))
                self._check(self._lib.mcmc_hip_set_mode_logdensities(self._h, _dp(am)))
        if self.emit_thin > 1 and "thin_carry" in st:
            self.set_thin_carry(st["thin_carry"])
        if self.n_functions and "ll_c" in st:   # (absent: every function is called at the next launch)
            self.set_component_loglikes(st["ll_c"])

    def carries_modes(self):
        """Mixtures in incremental mode: does the step kernel this configuration selects carry the
        log-density of every mode (mcmc_hip_incremental_carries_modes)?  The oracle takes the rule
        from here (`oracle.cbind.Problem(carry_modes=...)`)."""
        return bool(self.incremental and self._lib.mcmc_hip_incremental_carries_modes(self._h))

    def carries_periodic(self):
        """One mode with periodic parameters in incremental mode: the rule of step_inc_kernel<.., periodic>
        (wrap only what leaves [lo, hi), carried log-likelihood) applies
        (mcmc_hip_incremental_carries_periodic); the oracle takes it from here."""
        return bool(self.incremental and self._lib.mcmc_hip_incremental_carries_periodic(self._h))

    # -- sampling
    def step(self, n_steps):
        self._check(self._lib.mcmc_hip_step(self._h, int(n_steps)))

    def set_move(self, move, stretch_a=2.0):
        """The move `step` makes (mcmc_hip_set_move): "metropolis" (the default: the Gaussian
        proposal along Haar directions) or "stretch", the affine-invariant stretch move with scale
        `stretch_a` on the target of `set_target_function`.  A stretch step is two half-updates:
        the function is called twice per step, each time with the n_walkers / 2 trial rows of the
        active half of every group, in ascending walker order.  No proposal covariance is needed.
        What the move does not serve is refused by name at the first `step`."""
        kinds = {None: MOVE_METROPOLIS, "metropolis": MOVE_METROPOLIS, "stretch": MOVE_STRETCH}
        if move not in kinds:
            raise EngineError(ERR_ARG, f"move must be 'metropolis' or 'stretch', got {move!r}")
        self._check(self._lib.mcmc_hip_set_move(self._h, kinds[move], float(stretch_a)))

    def set_moves(self, moves):
        """A weighted mixture of ensemble moves in place of the one move (mcmc_hip_set_moves;
        cobaya_amd/moves.py has the format): e.g. [["de", 0.8], ["de", 0.2, {"gamma": 1.0}]].  The
        kind of a step is drawn once per step for the whole ensemble; halves, partners and limits
        are the stretch move's.  None or an empty list switches the mixture off."""
        from .moves import parse
        if not moves:
            self._check(self._lib.mcmc_hip_set_moves(self._h, 0, None, None, None, None))
            return
        try:
            members = parse(moves, self.d)
        except ValueError as e:
            raise EngineError(ERR_ARG, str(e)) from None
        kinds = np.array([m[0] for m in members], np.int32)
        w, p0, p1 = (np.array([m[i] for m in members], np.float64) for i in (1, 2, 3))
        self._check(self._lib.mcmc_hip_set_moves(self._h, len(members), _ip(kinds), _dp(w), _dp(p0), _dp(p1)))

    def sync(self):
        self._check(self._lib.mcmc_hip_sync(self._h))

    def counters(self):
        c = np.zeros(4, np.int64)
        self._check(self._lib.mcmc_hip_get_counters(self._h, c.ctypes.data_as(c_int64_p)))
        return {"steps": int(c[0]), "accepted": int(c[1]), "stuck": int(c[2]),
                "dropped_rows": int(c[3])}

    def drain_samples(self):
        n = C.c_int64()
        self._check(self._lib.mcmc_hip_drain_samples(self._h, None, 0, C.byref(n)))
        rows = np.empty((n.value, self.d + 5))
        if n.value:
            self._check(self._lib.mcmc_hip_drain_samples(self._h, _dp(rows), n.value,
                                                         C.byref(n)))
        return rows

    emit_thin = 1

    def set_emit_thin(self, thin):
        """Thinned emission on the device (mcmc_hip_set_emit_thin; collection.py:1373-1383): a
        walker's weights add up and a row is emitted when the sum reaches `thin`, with weight
        sum // thin.  Served by step_inc_kernel<.., emit>; other configurations refuse at their
        first step (EngineError): thin on the host then."""
        self._check(self._lib.mcmc_hip_set_emit_thin(self._h, int(thin)))
        self.emit_thin = int(thin)

    def get_thin_carry(self):
        out = np.empty(self.W, np.int32)
        self._check(self._lib.mcmc_hip_get_thin_carry(self._h, _ip(out)))
        return out

    def set_thin_carry(self, carry):
        c = np.ascontiguousarray(carry, dtype=np.int32)
        assert c.shape == (self.W,)
        self._check(self._lib.mcmc_hip_set_thin_carry(self._h, _ip(c)))

    def set_drain_slots(self, n_slots):
        self._check(self._lib.mcmc_hip_set_drain_slots(self._h, int(n_slots)))
        self.drain_slots = int(n_slots)

    drain_slots = 4

    def drain_samples_view(self):
        """The rows accumulated since the last drain as a READ-ONLY view of a pinned host slot
        the library owns: no host-side copy.  The view stays valid for `drain_slots - 1`
        further drains (then its slot is reused) and dies with the engine -- copy what must
        live longer."""
        p = c_double_p()
        n = C.c_int64()
        self._check(self._lib.mcmc_hip_drain_samples_pinned(self._h, C.byref(p), C.byref(n)))
        if not n.value:
            return np.empty((0, self.d + 5))
        rows = np.ctypeslib.as_array(p, shape=(n.value, self.d + 5))
        rows.flags.writeable = False
        return rows

    # -- moments
    def set_moment_shift(self, shift):
        shift = _f64(shift, (self.d,))
        self._check(self._lib.mcmc_hip_set_moment_shift(self._h, _dp(shift)))

    def accumulate_moments(self):
        self._check(self._lib.mcmc_hip_accumulate_moments(self._h))

    def read_moments(self, reset=False):
        n = C.c_int64()
        gs = np.empty((self.G, self.d))
        S = np.empty((self.d, self.d))
        self._check(self._lib.mcmc_hip_read_moments(self._h, C.byref(n), _dp(gs), _dp(S),
                                                    int(bool(reset))))
        return n.value, gs, S

    def set_moments(self, n_snapshots, group_sum, pooled_S):
        gs, S = _f64(group_sum, (self.G, self.d)), _f64(pooled_S, (self.d, self.d))
        self._check(self._lib.mcmc_hip_set_moments(self._h, int(n_snapshots), _dp(gs), _dp(S)))

    def request_moments(self):
        """Queue the read-out (and reset) of the moment accumulators and of the accept counter
        behind the work already in the stream; returns at once."""
        self._check(self._lib.mcmc_hip_request_moments(self._h))

    def fetch_moments(self):
        """(n_snapshots, group_sum[G][d], pooled_S[d][d], {"steps", "accepted"}) of the
        pending request; waits only for its copies, not for launches queued after it."""
        n = C.c_int64()
        gs = np.empty((self.G, self.d))
        S = np.empty((self.d, self.d))
        c = np.zeros(2, np.int64)
        self._check(self._lib.mcmc_hip_fetch_moments(self._h, C.byref(n), _dp(gs), _dp(S),
                                                     c.ctypes.data_as(c_int64_p)))
        return n.value, gs, S, {"steps": int(c[0]), "accepted": int(c[1])}

    # -- streaming marginal histograms
    def configure_marginals(self, dims1=(), bins1=128, pairs=(), bins2=32, lo=None, hi=None):
        """The histograms every `accumulate_marginals` adds the ensemble to (mcmc_hip_marginals_configure):
        `dims1` sampler indices with `bins1` bins each, `pairs` ordered (i, j) with `bins2` x `bins2`
        bins each, `lo` / `hi` [d] the fixed range of every parameter in use.  Nothing listed: off.
        With m derived rows configured an index d + r names row r of them, and `lo` / `hi` hold
        d + m entries."""
        dims1 = np.ascontiguousarray(dims1, dtype=np.int32).reshape(-1)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        n1, n2 = len(dims1), len(pairs)
        n = self.d + self.n_derived     # (indices from d up name the derived rows: configure_derived first)
        lo = _f64(lo, (n,)) if (n1 or n2) else None
        hi = _f64(hi, (n,)) if (n1 or n2) else None
        self._check(self._lib.mcmc_hip_marginals_configure(
            self._h, n1, _ip(dims1) if n1 else None, int(bins1), n2, _ip(pairs) if n2 else None,
            int(bins2), _dp(lo) if lo is not None else None, _dp(hi) if hi is not None else None))

    def marginals_layout(self):
        """{"n_counters", "n1", "bins1", "n2", "bins2", "offset_pairs"} of the slab
        (mcmc_hip_marginals_layout); n_counters == 0: the feature is off."""
        n, off = C.c_int64(), C.c_int64()
        v = [C.c_int32() for _ in range(4)]
        self._check(self._lib.mcmc_hip_marginals_layout(self._h, C.byref(n), C.byref(v[0]), C.byref(v[1]),
                                                        C.byref(v[2]), C.byref(v[3]), C.byref(off)))
        return {"n_counters": n.value, "n1": v[0].value, "bins1": v[1].value, "n2": v[2].value,
                "bins2": v[3].value, "offset_pairs": off.value}

    def accumulate_marginals(self):
        """Queue one accumulation: every walker of this process, once, into every histogram."""
        self._check(self._lib.mcmc_hip_marginals_accumulate(self._h))

    def request_marginals(self):
        """Queue the read-out and the reset of the slab behind the work already in the stream."""
        self._check(self._lib.mcmc_hip_marginals_request(self._h))

    def fetch_marginals(self):
        """(counts[n_counters] uint64, n_accumulations) of the pending request; waits for its copy
        only."""
        n = self.marginals_layout()["n_counters"]
        out = np.zeros(n, np.uint64)
        k = C.c_int64()
        self._check(self._lib.mcmc_hip_marginals_fetch(self._h, out.ctypes.data_as(c_uint64_p), n,
                                                       C.byref(k)))
        return out, k.value

    def marginals_set(self, counts, n_accumulations):
        """Restore the counts of an unfinished interval (resume)."""
        c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        self._check(self._lib.mcmc_hip_marginals_set(self._h, c.ctypes.data_as(c_uint64_p), len(c),
                                                     int(n_accumulations)))

    # -- derived parameters
    def configure_derived(self, m, cross_dims=(), shift=None):
        """`m` derived rows z[m][W] and their moments (mcmc_hip_derived_configure): `cross_dims` the
        sampler indices whose cross-moments are kept, `shift` [m] the conditioning vector (default
        zeros).  m = 0: off.  Before `configure_marginals`, whose indices d .. d + m - 1 name the rows."""
        m = int(m)
        cross = np.ascontiguousarray(cross_dims, dtype=np.int32).reshape(-1)
        sh = _f64(np.zeros(m) if shift is None else shift, (m,))
        self._check(self._lib.mcmc_hip_derived_configure(self._h, m, len(cross), _ip(cross) if len(cross) else None,
                                                         _dp(sh) if m else None))
        self.n_derived, self.n_derived_cross = m, (len(cross) if m else 0)
        self._derived_views = None

    def derived_set_group_size(self, group_size):
        """The groups of the derived sums (default: the engine's group_size): any divisor of W."""
        self._check(self._lib.mcmc_hip_derived_set_group_size(self._h, int(group_size)))

    def derived_layout(self):
        """{"m", "n_cross", "group_size", "n_accumulations"} (mcmc_hip_derived_layout); m == 0: off."""
        v = [C.c_int32() for _ in range(3)]
        n = C.c_int64()
        self._check(self._lib.mcmc_hip_derived_layout(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]),
                                                      C.byref(n)))
        return {"m": v[0].value, "n_cross": v[1].value, "group_size": v[2].value, "n_accumulations": n.value}

    def derived_buffers(self):
        """(device pointer of x[d][W], of z[m][W]): what a caller fills z from, on `stream_handle()`."""
        x, z = C.c_uint64(), C.c_uint64()
        self._check(self._lib.mcmc_hip_derived_buffers(self._h, C.byref(x), C.byref(z)))
        return x.value, z.value

    def derived_row_views(self):
        """(x rows, z rows, stream): zero-copy torch.float64 views of the d rows of x[d][W] and the m
        rows of z[m][W], each of shape (W,), and the engine's stream as a `torch.cuda.ExternalStream`.
        The views of x are for reading.  `import torch` before the first Engine is created."""
        if getattr(self, "_derived_views", None) is None:
            import torch
            dev = torch.device("cuda", int(self.cfg.device))
            try:
                stream = torch.cuda.ExternalStream(self.stream_handle(), device=dev)
            except RuntimeError as e:
                raise EngineError(ERR_DEVICE,
                                  f"PyTorch cannot use device {dev} in this process ({e}): `import torch` "
                                  "before the first Engine is created (before libmcmc_hip.so is loaded), so "
                                  "that both use one HIP runtime") from e
            xp, zp = self.derived_buffers()

            class _View:   # __cuda_array_interface__ of float64 at a device pointer: no copy
                def __init__(self, ptr, shape):
                    self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f8", "data": (ptr, False),
                                                     "version": 2, "strides": None}

            x = torch.as_tensor(_View(xp, (self.d, self.W)), device=dev)
            z = torch.as_tensor(_View(zp, (self.n_derived, self.W)), device=dev)
            self._derived_views = (list(x.unbind(0)), list(z.unbind(0)), stream)
        return self._derived_views

    def derived_set_values(self, values):
        """z from the host, point-major [W][m]."""
        v = _f64(values, (self.W, self.n_derived))
        self._check(self._lib.mcmc_hip_derived_set_values(self._h, _dp(v)))

    def derived_get_values(self):
        """z as it lies on the device (the stream is waited for), point-major [W][m]."""
        v = np.empty((self.W, self.n_derived))
        self._check(self._lib.mcmc_hip_derived_get_values(self._h, _dp(v)))
        return v

    def accumulate_derived(self):
        """Queue one accumulation of the moments of z as it is (two launches)."""
        self._check(self._lib.mcmc_hip_derived_accumulate(self._h))

    def request_derived(self):
        """Queue the read-out and the reset of the accumulators behind the work already in the stream."""
        self._check(self._lib.mcmc_hip_derived_request(self._h))

    def fetch_derived(self):
        """{"N", "A"[m], "B"[m (m + 1) / 2], "C"[m, n_cross], "X"[n_cross], "V"[n_cross], "bad"[m], "min"[m], "max"[m],
        "n"} of the pending request; waits for its copy only."""
        m, nc = self.n_derived, self.n_derived_cross
        N, n = C.c_uint64(), C.c_int64()
        A, B, Cc, X, V = np.zeros(m), np.zeros(m * (m + 1) // 2), np.zeros((m, nc)), np.zeros(nc), np.zeros(nc)
        bad, mn, mx = np.zeros(m, np.uint64), np.zeros(m), np.zeros(m)
        self._check(self._lib.mcmc_hip_derived_fetch(self._h, C.byref(N), _dp(A), _dp(B), _dp(Cc) if nc else None,
                                                     _dp(X) if nc else None, _dp(V) if nc else None, bad.ctypes.data_as(c_uint64_p), _dp(mn), _dp(mx), C.byref(n)))
        return {"N": int(N.value), "A": A, "B": B, "C": Cc, "X": X, "V": V, "bad": bad, "min": mn, "max": mx, "n": int(n.value)}

    def derived_set(self, part):
        """Restore the accumulators of an unfinished interval (resume): what `fetch_derived` returns."""
        m, nc = self.n_derived, self.n_derived_cross
        A, B = _f64(part["A"], (m,)), _f64(part["B"], (m * (m + 1) // 2,))
        Cc, X, V = _f64(part["C"], (m, nc)), _f64(part["X"], (nc,)), _f64(part["V"], (nc,))
        bad = np.ascontiguousarray(part["bad"], dtype=np.uint64).reshape(m)
        mn, mx = _f64(part["min"], (m,)), _f64(part["max"], (m,))
        self._check(self._lib.mcmc_hip_derived_set(self._h, int(part["N"]), _dp(A), _dp(B), _dp(Cc) if nc else None,
                                                   _dp(X) if nc else None, _dp(V) if nc else None, bad.ctypes.data_as(c_uint64_p), _dp(mn), _dp(mx), int(part["n"])))

    # -- lagged cross-products for the autocorrelation time
    def configure_autocorr(self, dims=(), lags=16):
        """The parameters (`dims`: distinct sampler indices) whose lagged cross-products with the
        previous `lags` accumulated snapshots every `accumulate_autocorr` adds
        (mcmc_hip_autocorr_configure).  Nothing listed: off."""
        dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1)
        self._check(self._lib.mcmc_hip_autocorr_configure(
            self._h, len(dims), _ip(dims) if len(dims) else None, int(lags)))

    def autocorr_layout(self):
        """{"n_dims", "lags", "n_doubles", "held"} (mcmc_hip_autocorr_layout); all zero: off."""
        n, L, held, nd = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._lib.mcmc_hip_autocorr_layout(self._h, C.byref(n), C.byref(L), C.byref(nd),
                                                       C.byref(held)))
        return {"n_dims": n.value, "lags": L.value, "n_doubles": nd.value, "held": held.value}

    def accumulate_autocorr(self):
        """Queue one accumulation: the ensemble as it is becomes the ring's newest snapshot and is
        multiplied with every snapshot the ring holds."""
        self._check(self._lib.mcmc_hip_autocorr_accumulate(self._h))

    def request_autocorr(self):
        """Queue the read-out and the zeroing of the accumulators behind the work already in the
        stream; the ring is kept."""
        self._check(self._lib.mcmc_hip_autocorr_request(self._h))

    def fetch_autocorr(self):
        """(sums[3][lags + 1][n_dims] (P, A, B), n_pairs[lags + 1] int64) of the pending request;
        waits for its copy only."""
        lay = self.autocorr_layout()
        out = np.zeros((3, lay["lags"] + 1, lay["n_dims"]), np.float64)
        k = np.zeros(lay["lags"] + 1, np.int64)
        self._check(self._lib.mcmc_hip_autocorr_fetch(self._h, _dp(out), out.size,
                                                      k.ctypes.data_as(c_int64_p)))
        return out, k

    def autocorr_set(self, sums, n_pairs):
        """Restore open accumulators (resume); the ring is not restored."""
        s = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
        k = np.ascontiguousarray(n_pairs, dtype=np.int64).reshape(-1)
        if len(k) != self.autocorr_layout()["lags"] + 1:
            raise EngineError(ERR_ARG, "autocorr_set: n_pairs holds %d counts, not lags + 1" % len(k))
        self._check(self._lib.mcmc_hip_autocorr_set(self._h, _dp(s), len(s), k.ctypes.data_as(c_int64_p)))

    def autocorr_reset(self):
        """Empty the ring: the next accumulation pairs with itself only."""
        self._check(self._lib.mcmc_hip_autocorr_reset(self._h))

    # -- best fit, MAP and profile likelihoods
    def configure_bestfit(self, dims=(), bins=64, lo=None, hi=None, quantity="loglike"):
        """The two records (map, bestfit) and the profiles every `accumulate_bestfit` takes the
        ensemble into (mcmc_hip_bestfit_configure): `dims` sampler indices with `bins` bins each
        over `lo` / `hi` [d], the profiled `quantity` "loglike" or "logpost".  No dims: the records
        only."""
        if quantity not in BESTFIT_QUANTITIES:
            raise EngineError(ERR_ARG, "configure_bestfit: quantity must be one of %r, got %r"
                              % (BESTFIT_QUANTITIES, quantity))
        dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1)
        n = len(dims)
        lo = _f64(lo, (self.d,)) if n else None
        hi = _f64(hi, (self.d,)) if n else None
        self._check(self._lib.mcmc_hip_bestfit_configure(
            self._h, n, _ip(dims) if n else None, int(bins), _dp(lo) if n else None,
            _dp(hi) if n else None, BESTFIT_QUANTITIES.index(quantity)))

    def bestfit_layout(self):
        """{"on", "n", "bins", "quantity", "n_slab", "n_records"} (mcmc_hip_bestfit_layout);
        on == 0: the feature is off."""
        v = [C.c_int32() for _ in range(4)]
        ns, nr = C.c_int64(), C.c_int64()
        self._check(self._lib.mcmc_hip_bestfit_layout(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]),
                                                      C.byref(v[3]), C.byref(ns), C.byref(nr)))
        return {"on": v[0].value, "n": v[1].value, "bins": v[2].value,
                "quantity": BESTFIT_QUANTITIES[v[3].value], "n_slab": ns.value, "n_records": nr.value}

    def accumulate_bestfit(self):
        """Queue one accumulation: every walker of this process, once, into the profiles and the
        two records."""
        self._check(self._lib.mcmc_hip_bestfit_accumulate(self._h))

    def request_bestfit(self):
        """Queue the read-out and the emptying of slab and records behind the work already in the
        stream."""
        self._check(self._lib.mcmc_hip_bestfit_request(self._h))

    def fetch_bestfit(self):
        """(slab[n, bins] uint64 keys, records[2, 6 + d] uint64 words, n_accumulations) of the
        pending request; waits for its copy only."""
        lay = self.bestfit_layout()
        slab = np.zeros((lay["n"], lay["bins"]), np.uint64)
        rec = np.zeros((2, lay["n_records"] // 2), np.uint64)
        k = C.c_int64()
        self._check(self._lib.mcmc_hip_bestfit_fetch(
            self._h, slab.ctypes.data_as(c_uint64_p), slab.size, rec.ctypes.data_as(c_uint64_p), rec.size,
            C.byref(k)))
        return slab, rec, k.value

    def bestfit_set(self, slab, records, n_accumulations):
        """Restore slab and records of an unfinished interval (resume)."""
        s = np.ascontiguousarray(slab, dtype=np.uint64).reshape(-1)
        r = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1)
        self._check(self._lib.mcmc_hip_bestfit_set(
            self._h, s.ctypes.data_as(c_uint64_p), len(s), r.ctypes.data_as(c_uint64_p), len(r),
            int(n_accumulations)))

    # -- evidence: the sums of the ellipsoid-truncated harmonic mean
    def configure_evidence(self, r2=()):
        """The radii (R^2, ascending; 1..8 of them) whose sums every `accumulate_evidence` adds to
        (mcmc_hip_evidence_configure).  None listed: off, everything is freed."""
        r2 = np.ascontiguousarray(r2, dtype=np.float64).reshape(-1)
        self._check(self._lib.mcmc_hip_evidence_configure(self._h, len(r2), _dp(r2) if len(r2) else None))

    def evidence_layout(self):
        """{"on", "n_radii", "n_groups", "n_ell", "active", "staged", "n_accumulations"}
        (mcmc_hip_evidence_layout); all zero: off."""
        v = [C.c_int32() for _ in range(5)]
        ne, na = C.c_int64(), C.c_int64()
        self._check(self._lib.mcmc_hip_evidence_layout(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]),
                                                       C.byref(ne), C.byref(v[3]), C.byref(v[4]), C.byref(na)))
        return {"on": v[0].value, "n_radii": v[1].value, "n_groups": v[2].value, "n_ell": ne.value,
                "active": v[3].value, "staged": v[4].value, "n_accumulations": na.value}

    def evidence_set_ellipsoid(self, centre, covmat):
        """Hand in an ellipsoid as (m[d], C[d][d]); the library forms the inverse of chol(C).  The
        first one becomes active at once, with c = the maximum of logpost; a later one is staged
        until the next closing request."""
        self._check(self._lib.mcmc_hip_evidence_set_ellipsoid(
            self._h, _dp(_f64(centre, (self.d,))), _dp(_f64(covmat, (self.d, self.d)))))

    def accumulate_evidence(self):
        """Queue one accumulation: every walker of this process, once, under the active ellipsoid."""
        self._check(self._lib.mcmc_hip_evidence_accumulate(self._h))

    def request_evidence(self, close=True):
        """Queue the read-out behind the work already in the stream.  `close`: also zero the sums
        and activate a staged ellipsoid, in stream order (False: nothing is disturbed)."""
        self._check(self._lib.mcmc_hip_evidence_request(self._h, 1 if close else 0))

    def fetch_evidence(self):
        """{"sums" [G, n_radii] float64, "counts" [G, n_radii] uint64, "clamped", "n",
        "active", "staged"} of the pending request; an ellipsoid is the flat m[d] | Linv[d][d] | c
        or None; waits for the copy only."""
        lay = self.evidence_layout()
        shape = (lay["n_groups"], lay["n_radii"])
        sums, counts = np.zeros(shape), np.zeros(shape, np.uint64)
        act, stg = np.zeros(lay["n_ell"]), np.zeros(lay["n_ell"])
        cl, k, ha, hs = C.c_uint64(), C.c_int64(), C.c_int32(), C.c_int32()
        self._check(self._lib.mcmc_hip_evidence_fetch(
            self._h, _dp(sums), counts.ctypes.data_as(c_uint64_p), sums.size, C.byref(cl), C.byref(k),
            _dp(act), _dp(stg), lay["n_ell"], C.byref(ha), C.byref(hs)))
        return {"sums": sums, "counts": counts, "clamped": int(cl.value), "n": int(k.value),
                "active": act if ha.value else None, "staged": stg if hs.value else None}

    def evidence_set(self, sums, counts, clamped, n_accumulations, active=None, staged=None):
        """Restore the sums of an unfinished interval and the ellipsoids (resume)."""
        s = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
        c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        n_ell = self.d * (self.d + 1) + 1
        act = None if active is None else _f64(active, (n_ell,))
        stg = None if staged is None else _f64(staged, (n_ell,))
        self._check(self._lib.mcmc_hip_evidence_set(
            self._h, _dp(s), c.ctypes.data_as(c_uint64_p), len(s) if len(s) == len(c) else -1, int(clamped),
            int(n_accumulations), None if act is None else _dp(act), None if stg is None else _dp(stg), n_ell))

    # -- importance reweighting: the weighted sums under exp(log-weight)
    def configure_importance(self, cov=()):
        """One alternative per entry of `cov` (1..8; truthy: the full weighted covariance is kept, d <=
        128) whose sums every `accumulate_importance` adds to (mcmc_hip_importance_configure).  None
        listed: off, everything is freed."""
        cov = np.ascontiguousarray([1 if c else 0 for c in cov], dtype=np.int32)
        self._check(self._lib.mcmc_hip_importance_configure(self._h, len(cov), _ip(cov) if len(cov) else None))
        self._importance_views = None

    def importance_set_group_size(self, group_size):
        """The groups of the importance sums (default: the engine's group_size): any divisor of W.  The
        sums are dropped."""
        self._check(self._lib.mcmc_hip_importance_set_group_size(self._h, int(group_size)))

    def importance_layout(self):
        """{"n_alt", "n_groups", "n_sums", "offsets" [n_alt], "cov" [n_alt], "n_accumulations", "x_ptr"}
        (mcmc_hip_importance_layout); n_alt == 0: off."""
        na, ng = C.c_int32(), C.c_int32()
        ns, nacc, xp = C.c_int64(), C.c_int64(), C.c_uint64()
        off, cov = np.zeros(8, np.int64), np.zeros(8, np.int32)
        self._check(self._lib.mcmc_hip_importance_layout(self._h, C.byref(na), C.byref(ng), C.byref(ns),
                                                         off.ctypes.data_as(c_int64_p), _ip(cov), C.byref(nacc),
                                                         C.byref(xp)))
        return {"n_alt": na.value, "n_groups": ng.value, "n_sums": ns.value, "offsets": off[:na.value].tolist(),
                "cov": cov[:na.value].tolist(), "n_accumulations": nacc.value, "x_ptr": xp.value}

    def importance_row_views(self):
        """(x rows, delta, stream): zero-copy torch.float64 views of the d rows of x[d][W], each of
        shape (W,) and for reading; the log-weights delta[n_alt][W], a tensor of the caller's to fill;
        and the engine's stream as a `torch.cuda.ExternalStream`.  `import torch` before the first
        Engine is created."""
        if getattr(self, "_importance_views", None) is None:
            import torch
            dev = torch.device("cuda", int(self.cfg.device))
            try:
                stream = torch.cuda.ExternalStream(self.stream_handle(), device=dev)
            except RuntimeError as e:
                raise EngineError(ERR_DEVICE,
                                  f"PyTorch cannot use device {dev} in this process ({e}): `import torch` "
                                  "before the first Engine is created (before libmcmc_hip.so is loaded), so "
                                  "that both use one HIP runtime") from e
            lay = self.importance_layout()

            class _View:   # __cuda_array_interface__ of float64 at a device pointer: no copy
                def __init__(self, ptr, shape):
                    self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f8", "data": (ptr, False),
                                                     "version": 2, "strides": None}

            x = torch.as_tensor(_View(lay["x_ptr"], (self.d, self.W)), device=dev)
            with torch.cuda.stream(stream):
                delta = torch.zeros((lay["n_alt"], self.W), dtype=torch.float64, device=dev)
            self._importance_views = (list(x.unbind(0)), delta, stream)
        return self._importance_views

    def accumulate_importance(self, delta):
        """Queue one accumulation of the log-weights `delta` [n_alt][W] (a contiguous torch.float64
        tensor on the engine's device, filled on its stream) against the state as it is."""
        n_alt = self.importance_layout()["n_alt"]
        if tuple(delta.shape) != (n_alt, self.W) or not delta.is_contiguous() or delta.element_size() != 8 \
                or not delta.is_cuda or not delta.dtype.is_floating_point:
            raise EngineError(ERR_ARG, f"accumulate_importance: delta must be a contiguous torch.float64 tensor of "
                                       f"shape ({n_alt}, {self.W}) on the device, got {tuple(delta.shape)} "
                                       f"{delta.dtype} on {delta.device}")
        self._check(self._lib.mcmc_hip_importance_accumulate(self._h, int(delta.data_ptr())))

    def request_importance(self, close=True):
        """Queue the read-out behind the work already in the stream.  `close`: also zero the sums, in
        stream order (False: nothing is disturbed)."""
        self._check(self._lib.mcmc_hip_importance_request(self._h, 1 if close else 0))

    def fetch_importance(self):
        """{"sums" [n_sums] float64 (alternative k: [G][n_chains_k] at offsets[k]), "n" [n_alt, G]
        uint64, "counters" [n_alt, 3] uint64 (zero, nonfinite, clamped), "c" [n_alt], "n_acc"} of the
        pending request; waits for the copy only."""
        lay = self.importance_layout()
        sums = np.zeros(lay["n_sums"])
        n = np.zeros((lay["n_alt"], lay["n_groups"]), np.uint64)
        cnt, c, k = np.zeros((lay["n_alt"], 3), np.uint64), np.zeros(lay["n_alt"]), C.c_int64()
        self._check(self._lib.mcmc_hip_importance_fetch(
            self._h, _dp(sums), sums.size, n.ctypes.data_as(c_uint64_p), n.size, cnt.ctypes.data_as(c_uint64_p),
            _dp(c), C.byref(k)))
        return {"sums": sums, "n": n, "counters": cnt, "c": c, "n_acc": int(k.value)}

    def importance_set(self, part):
        """Restore the sums of an unfinished interval (resume): a dict as `fetch_importance` gives."""
        s = np.ascontiguousarray(part["sums"], dtype=np.float64).reshape(-1)
        n = np.ascontiguousarray(part["n"], dtype=np.uint64).reshape(-1)
        cnt = np.ascontiguousarray(part["counters"], dtype=np.uint64).reshape(-1)
        c = np.ascontiguousarray(part["c"], dtype=np.float64).reshape(-1)
        n_alt = self.importance_layout()["n_alt"]
        ok = len(cnt) == 3 * n_alt and len(c) == n_alt
        self._check(self._lib.mcmc_hip_importance_set(
            self._h, _dp(s), len(s) if ok else -1, n.ctypes.data_as(c_uint64_p), len(n),
            cnt.ctypes.data_as(c_uint64_p), _dp(c), int(part["n_acc"])))

    # -- ... and their reweighted marginal histograms (128-bit fixed-point counters as words lo, hi)
    def configure_importance_hist(self, on):
        """`on` [n_alt]: truthy where the alternative keeps a weighted copy of the histograms of
        `configure_marginals` (mcmc_hip_importance_hist_configure); after `configure_importance` and
        `configure_marginals`.  None truthy: off, everything is freed."""
        on = np.ascontiguousarray([1 if v else 0 for v in on], dtype=np.int32)
        n_alt = self.importance_layout()["n_alt"]
        if len(on) != n_alt:
            raise EngineError(ERR_ARG, f"configure_importance_hist: {len(on)} flags for {n_alt} alternatives")
        self._check(self._lib.mcmc_hip_importance_hist_configure(self._h, _ip(on) if len(on) else None))

    def importance_hist_layout(self):
        """{"n_hist", "on" [n_alt], "n_counters", "n_words"} (mcmc_hip_importance_hist_layout); n_words
        == 0: off.  The slab: per alternative with histograms, ascending, lo[n_counters] |
        hi[n_counters]; behind them saturated[n_hist]."""
        nh, nc, nw, on = C.c_int32(), C.c_int64(), C.c_int64(), np.zeros(8, np.int32)
        self._check(self._lib.mcmc_hip_importance_hist_layout(self._h, C.byref(nh), _ip(on), C.byref(nc), C.byref(nw)))
        return {"n_hist": nh.value, "on": [bool(v) for v in on[:self.importance_layout()["n_alt"]]],
                "n_counters": nc.value, "n_words": nw.value}

    def fetch_importance_hist(self):
        """{"lo", "hi" [n_hist, n_counters] uint64, "saturated" [n_hist] uint64, "n_acc"} of the last
        `request_importance`; waits for the copy only."""
        lay = self.importance_hist_layout()
        lo = np.zeros((lay["n_hist"], lay["n_counters"]), np.uint64)
        hi, sat, k = np.zeros_like(lo), np.zeros(lay["n_hist"], np.uint64), C.c_int64()
        self._check(self._lib.mcmc_hip_importance_hist_fetch(
            self._h, lo.ctypes.data_as(c_uint64_p), hi.ctypes.data_as(c_uint64_p), lo.size,
            sat.ctypes.data_as(c_uint64_p), C.byref(k)))
        return {"lo": lo, "hi": hi, "saturated": sat, "n_acc": int(k.value)}

    def importance_hist_set(self, part):
        """Restore the histograms of an unfinished interval (resume): a dict as `fetch_importance_hist`
        gives, behind `importance_set`, which carries c and the accumulations."""
        lo = np.ascontiguousarray(part["lo"], dtype=np.uint64).reshape(-1)
        hi = np.ascontiguousarray(part["hi"], dtype=np.uint64).reshape(-1)
        sat = np.ascontiguousarray(part["saturated"], dtype=np.uint64).reshape(-1)
        ok = len(lo) == len(hi) and len(sat) == self.importance_hist_layout()["n_hist"]
        self._check(self._lib.mcmc_hip_importance_hist_set(
            self._h, lo.ctypes.data_as(c_uint64_p), hi.ctypes.data_as(c_uint64_p), len(lo) if ok else -1,
            sat.ctypes.data_as(c_uint64_p)))

    # -- the checkpoint on the device
    def checkpoint_set_ring(self, intervals=(), min_capacity=16, first_index=0):
        """`intervals`: the (n_snapshots, group_sum[G][d], pooled_S[d][d]) the caller still
        holds, oldest first (none at the start of a run).  (`first_index`, the run's index of the
        first of them, is of no use to the device, which sums a window slot by slot.)"""
        n = len(intervals)
        gs = _f64(np.array([iv[1] for iv in intervals]).reshape(n, self.G * self.d)) if n else None
        S = _f64(np.array([iv[2] for iv in intervals]).reshape(n, self.d * self.d)) if n else None
        self._check(self._lib.mcmc_hip_checkpoint_set_ring(
            self._h, n, _dp(gs) if n else None, _dp(S) if n else None, int(min_capacity)))
        self.ckpt_capacity = 16
        while self.ckpt_capacity < max(n + 2, int(min_capacity)):
            self.ckpt_capacity *= 2

    def checkpoint_set_accepted(self, accepted):
        self._check(self._lib.mcmc_hip_checkpoint_set_accepted(self._h, int(accepted)))

    def checkpoint_begin(self, n_window_intervals, n_window_snapshots, steps_since):
        """-> (device pointer, length in doubles) of the buffer an all-reduce carries."""
        ptr, n = C.c_uint64(), C.c_int32()
        self._check(self._lib.mcmc_hip_checkpoint_begin(
            self._h, int(n_window_intervals), int(n_window_snapshots), float(steps_since),
            C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def checkpoint_solve(self, learn_lo, learn_hi):
        self._check(self._lib.mcmc_hip_checkpoint_solve(self._h, float(learn_lo), float(learn_hi)))

    def checkpoint_fetch(self):
        st = np.zeros(8)
        cov = np.empty((self.d, self.d))
        self._check(self._lib.mcmc_hip_checkpoint_fetch(self._h, _dp(st), _dp(cov)))
        return {"Rminus1_groups": st[0], "status": int(st[1]), "refreshed": bool(st[2]),
                "n_chains": st[3], "sum_N": st[4], "d_accepted": st[5], "d_steps": st[6],
                "accepted": st[7], "mean_of_covs": cov}

    def checkpoint_request_payload(self):
        """Instead of `checkpoint_solve`: queue the read-out of the (all-reduced) payload; the
        caller solves it on the host while the next launch runs."""
        self._check(self._lib.mcmc_hip_checkpoint_request_payload(self._h))

    def checkpoint_fetch_payload(self):
        """The payload of the pending request: [chains, sum N, accepted since, steps x walkers
        since, accepted | sum N cov | sum of chain means | sum of m m^T]."""
        n = 5 + 2 * self.d * self.d + self.d
        out = np.empty(n)
        self._check(self._lib.mcmc_hip_checkpoint_fetch_payload(self._h, _dp(out), n))
        return out

    # -- R-1 of the confidence bounds on the device
    BOUNDS_MAX_SLOTS = 64

    def bounds_configure(self, n_slots):
        """Ring of `n_slots` ensemble snapshots [slot][d][W] on the device (0 frees it)."""
        self._check(self._lib.mcmc_hip_bounds_configure(self._h, int(n_slots)))

    def bounds_snapshot(self, slot):
        """The current points -> ring slot, in stream order."""
        self._check(self._lib.mcmc_hip_bounds_snapshot(self._h, int(slot)))

    def bounds_statistics(self, slots, limfrac, want_bounds=False):
        """Per chain and parameter the lower / upper bound GetDist's `confidence(i, limfrac,
        upper)` gives for the samples in `slots`; returns the [1 + 4 d] sums over the chains of
        all ranks the statistic is formed from (and this rank's bounds [G][d][2] on request)."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        stats = np.empty(1 + 4 * self.d)
        b = np.empty((self.G, self.d, 2)) if want_bounds else None
        self._check(self._lib.mcmc_hip_bounds_statistics(
            self._h, len(sl), _ip(sl), float(limfrac), _dp(stats), _dp(b) if want_bounds else None))
        return (stats, b) if want_bounds else stats

    def bounds_get_slot(self, slot):
        x = np.empty((self.W, self.d))
        self._check(self._lib.mcmc_hip_bounds_get_slot(self._h, int(slot), _dp(x)))
        return x

    def bounds_set_slot(self, slot, x):
        x = _f64(x, (self.W, self.d))
        self._check(self._lib.mcmc_hip_bounds_set_slot(self._h, int(slot), _dp(x)))

    def stream_handle(self):
        return int(self._lib.mcmc_hip_stream_handle(self._h))

    def set_comm(self, comm):
        """Attach the shards' communicator: `checkpoint_begin` then all-reduces its payload over
        it, in place and in stream order.  The communicator must outlive the engine."""
        self._check(self._lib.mcmc_hip_set_comm(self._h, comm.handle if comm is not None else None))
        self._comm = comm
        self.comm_attached = comm is not None

    comm_attached = False

    # -- timing
    def enable_timing(self, on=True):
        self._check(self._lib.mcmc_hip_enable_timing(self._h, int(bool(on))))

    def last_step_kernel(self):
        """Name of the step kernel the last `step` launched, as its launcher reports it."""
        return self._lib.mcmc_hip_last_step_kernel(self._h).decode()

    def kernel_times(self, reset=False):
        ms = np.zeros(3)
        n = C.c_int64()
        self._check(self._lib.mcmc_hip_kernel_times(self._h, _dp(ms), C.byref(n),
                                                    int(bool(reset))))
        return {"step_ms": ms[0], "basis_ms": ms[1], "moments_ms": ms[2],
                "step_launches": n.value}
