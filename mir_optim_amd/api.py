"""ctypes binding of libmir_optim_amd.so, mirroring the reference's D API for the
`mir.optim.least_squares` path (names, argument meaning, error behaviour):

  reference (source/mir/optim/least_squares.d)          here
  ---------------------------------------------------   ------------------------------------
  LeastSquaresStatus                LS:20-46            LeastSquaresStatus
  LeastSquaresSettings!T            LS:85-123           LeastSquaresSettings(dtype)
  LeastSquaresResult!T              LS:128-143          LeastSquaresResult
  optimize!(f, g, tm) (throws)      LS:165-215          optimize(...)      raises LeastSquaresException
  optimizeLeastSquares!(f, g, tm)   LS:459-519          optimizeLeastSquares(...)
  leastSquaresStatusString          LS:528-557          leastSquaresStatusString
  mir_least_squares_*_length        LS:642-656          mir_least_squares_work_length / _iwork_length
  solveBoxQP (boxcqp.d:85-102)                          solveBoxQP(...)
  BoxQPSettings!T (boxcqp.d:56-71)                      BoxQPSettings(dtype)

No arithmetic happens in Python. The HIP library is mandatory: a missing library raises at
import time, and a missing GPU makes every solve return status numericError (never a CPU path).
"""
import ctypes as C
import enum
import os
import types

import numpy as np

from . import build as _build

__all__ = [
    "LeastSquaresStatus", "BoxQPStatus", "LeastSquaresSettings", "LeastSquaresResult", "BoxQPSettings",
    "LeastSquaresException", "optimize", "optimizeLeastSquares", "solveBoxQP", "leastSquaresStatusString",
    "mir_least_squares_work_length", "mir_least_squares_iwork_length", "mir_box_qp_work_length",
    "mir_box_qp_iwork_length", "GpuOptions", "Stats", "lib", "workloads_lib", "device_count",
    "DeviceBuffer", "Stream", "jtj", "fd_jtj", "DEVICE_CALLBACKS", "TIME_KERNELS", "optimizeLeastSquaresBatched", "batchedPosvx", "predictBatched", "BATCHED_ANALYTIC_JACOBIAN", "BATCHED_NO_LADDER", "BATCHED_DEVICE_BOUNDS",
    "solveBoxQPBatched", "solveBoxQPBatchedWide", "BOX_QP_UNCONSTRAINED_SOLUTION",
    "MODEL_EXP_DECAY", "MODEL_EXP3_AFFINE", "MODEL_EXP_DECAY_PAD8", "MODEL16_EXP_HARM16", "MODEL16_GAUSS3_AFFINE", "batched16JtJ", "optimizeLeastSquaresBatched16", "ResultS", "Trace", "TraceRecord", "Spline", "FitSplineResult", "fitSpline",
    "fit_spline_residuals", "variant_lr_cap",
    "VARIANT_BROYDEN_REWRITE", "VARIANT_FD_SEPARATE_FILL", "VARIANT_NO_SPECULATION", "VARIANT_NO_NULL_SKIP",
    "VARIANT_SOLVE_BOUNDED", "VARIANT_DEBUG_SOLVE", "VARIANT_HOST_PROFILE", "VARIANT_SOLVE_GENERIC", "VARIANT_SOLVE_ONE_WORKGROUP", "VARIANT_DEBUG_HELPERS_ABSENT", "VARIANT_FD_HOST_COLUMNS",
    "VARIANT_NO_PIPELINE", "FD_BASE_POINT", "VARIANT_NO_FD_BASE_POINT", "VARIANT_FD_WRITE_J", "BatchedOptions", "BatchedExtras", "BATCHED_ABSOLUTE_SIGMA", "BATCHED_BOUNDS_PER_PROBLEM",
    "covariance", "spdInverse", "COVARIANCE_ABSOLUTE_SIGMA",
    "fitSplineGpu", "splineEvalGpu", "fit_spline_eval_gpu", "fit_spline_eval_host", "fit_spline_factor",
    "lmSolve", "lm_solve_class",
    "lrPass", "lrFlush", "lr_class", "lr_blocks", "lr_len",
    "lm_state_dtype", "lmDecide", "fdPoints", "fdFill", "entryState", "sumsq_blocks", "unpackGrad",
]

MODEL_EXP_DECAY = 0      # n = 3: p0 exp(-t p1) + p2
MODEL_EXP3_AFFINE = 1    # n = 8: p0 exp(-t p1) + p2 exp(-t p3) + p4 exp(-t p5) + p6 + p7 t
MODEL_EXP_DECAY_PAD8 = 2  # n = 8: p0 exp(-t p1) + p2 + p3 sin 2t + p4 cos 2t + p5 sin 5t + p6 cos 5t + p7 t   (cfg 5)
# models of the 9 .. 16 parameter entries (mir_optimize_least_squares_batched16_d; double only)
MODEL16_EXP_HARM16 = 16     # n = 16: p0 exp(-t p1) + p2 + sum_{j=3..15} p_j h_j(t), h_j = sin / cos((j - 1) // 2 * pi / 2 * t) for odd / even j
MODEL16_GAUSS3_AFFINE = 17  # n = 11: sum_{k<3} p_3k exp(-((t - p_3k+1) / p_3k+2)^2 / 2) + p9 + p10 t
_MODELS16 = (MODEL16_EXP_HARM16, MODEL16_GAUSS3_AFFINE)

DEVICE_CALLBACKS = 1
TIME_KERNELS = 2
FD_BASE_POINT = 4        # MIR_LSQ_FD_BASE_POINT: the fbRowMajorDiff callback also takes p = 2n + 1 (panel + one residual vector)

# MIR_LSQ_VARIANT_* (include/mir_optim_amd.h): literal restatements the tests compare the product path with, and
# diagnostics; 0 = the product path
VARIANT_BROYDEN_REWRITE = 1 << 0
VARIANT_FD_SEPARATE_FILL = 1 << 1
VARIANT_NO_SPECULATION = 1 << 4
VARIANT_NO_NULL_SKIP = 1 << 5
VARIANT_SOLVE_BOUNDED = 1 << 6
VARIANT_DEBUG_SOLVE = 1 << 7
VARIANT_HOST_PROFILE = 1 << 8
VARIANT_SOLVE_GENERIC = 1 << 10
VARIANT_SOLVE_ONE_WORKGROUP = 1 << 11
VARIANT_DEBUG_HELPERS_ABSENT = 1 << 12
VARIANT_FD_HOST_COLUMNS = 1 << 13
VARIANT_NO_FD_BASE_POINT = 1 << 14
VARIANT_FD_WRITE_J = 1 << 15
VARIANT_NO_PIPELINE = 1 << 22


def variant_lr_cap(k):
    """Fold the pending Broyden terms into J after k (1..16) updates."""
    return (int(k) & 31) << 16


class LeastSquaresStatus(enum.IntEnum):  # LS:20-46
    maxIterations = -1
    furtherImprovement = 0
    xConverged = 1
    gConverged = 2
    fConverged = 3
    badBounds = -32
    badGuess = -31
    badMinStepQuality = -30
    badGoodStepQuality = -29
    badStepQuality = -28
    badLambdaParams = -27
    numericError = -26


class BoxQPStatus(enum.IntEnum):  # boxcqp.d:18-26
    solved = 0
    numericError = 1
    maxIterations = 2


class LeastSquaresException(Exception):
    """optimize() raises this for status < 0, like LS:175-179 ("mir-optim Least Squares: " ~ status string)."""

    def __init__(self, status, result=None):
        self.status = LeastSquaresStatus(status)
        self.result = result
        super().__init__("mir-optim Least Squares: " + leastSquaresStatusString(status))


class _QPd(C.Structure):
    _fields_ = [("relTolerance", C.c_double), ("absTolerance", C.c_double), ("maxIterations", C.c_uint32)]


class _QPs(C.Structure):
    _fields_ = [("relTolerance", C.c_float), ("absTolerance", C.c_float), ("maxIterations", C.c_uint32)]


_FIELDS = ["jacobianEpsilon", "absTolerance", "relTolerance", "gradTolerance", "maxGoodResidual", "maxStep",
           "maxLambda", "minLambda", "minStepQuality", "goodStepQuality", "lambdaIncrease", "lambdaDecrease"]


class _Sd(C.Structure):
    _fields_ = ([("maxIterations", C.c_uint32), ("maxAge", C.c_uint32)] + [(k, C.c_double) for k in _FIELDS]
                + [("qpSettings", _QPd)])


class _Ss(C.Structure):
    _fields_ = ([("maxIterations", C.c_uint32), ("maxAge", C.c_uint32)] + [(k, C.c_float) for k in _FIELDS]
                + [("qpSettings", _QPs)])


class _Rd(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_uint32), ("fCalls", C.c_uint32), ("gCalls", C.c_uint32),
                ("residual", C.c_double), ("lambda_", C.c_double)]


class _Rs(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_uint32), ("fCalls", C.c_uint32), ("gCalls", C.c_uint32),
                ("residual", C.c_float), ("lambda_", C.c_float)]


ResultS = _Rs


class _SliceD(C.Structure):
    _fields_ = [("length", C.c_size_t), ("ptr", C.c_void_p)]


class _Task(C.Structure):
    _fields_ = [("context", C.c_void_p), ("function", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("passes", C.c_uint64), ("accepted", C.c_uint64), ("rejected", C.c_uint64),
                ("step_guard_rejects", C.c_uint64), ("jacobian_full", C.c_uint64), ("jacobian_broyden", C.c_uint64),
                ("jtj_launches", C.c_uint64), ("jtj_broyden_launches", C.c_uint64), ("jtj_ms", C.c_double),
                ("jtj_broyden_ms", C.c_double), ("solve_ms", C.c_double), ("solve_launches", C.c_uint64),
                ("fd_ms", C.c_double), ("total_ms", C.c_double), ("qp_active_set_passes", C.c_uint64),
                ("broyden_lr_columns", C.c_uint64),
                ("jtj_fd_ms", C.c_double), ("jtj_fd_launches", C.c_uint64),
                ("elided_evaluations", C.c_uint64),
                ("allreduce_calls", C.c_uint64 * 3), ("allreduce_elems", C.c_uint64 * 3),
                ("broyden_flushes", C.c_uint64), ("jtj_resyncs", C.c_uint64),
                ("fd_callback_ms", C.c_double), ("fd_callback_calls", C.c_uint64), ("fd_callback_points", C.c_uint64),
                ("trial_callback_ms", C.c_double), ("trial_callback_calls", C.c_uint64),
                ("trial_callback_points", C.c_uint64),
                ("library_launches", C.c_uint64), ("round_launches", C.c_uint64 * 3), ("rounds", C.c_uint64 * 3),
                ("fd_host_wall_ms", C.c_double), ("fd_host_f_ms", C.c_double), ("fd_host_columns", C.c_uint64),
                ("host_f_ms", C.c_double), ("host_f_calls", C.c_uint64),
                ("fused_rounds", C.c_uint64), ("fused_passes", C.c_uint64), ("coop_timeouts", C.c_uint64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if isinstance(getattr(self, k), C.Array) else getattr(self, k)) for k, _ in self._fields_}


class TraceRecord(C.Structure):
    _fields_ = [("event", C.c_int32), ("iterations", C.c_uint32), ("lambda_", C.c_double), ("residual", C.c_double),
                ("trial_residual", C.c_double), ("dx_dot", C.c_double)]


class _TraceHeader(C.Structure):
    _fields_ = [("records", C.POINTER(TraceRecord)), ("capacity", C.c_uint64), ("count", C.c_uint64)]


class Trace:
    """mir_lsq_trace: per-pass records (event, iterations, lambda, residual, trial_residual, dx_dot)."""

    EVENTS = {0: "jacobian_full", 1: "jacobian_broyden", 2: "rejected", 3: "accepted", 4: "step_guard"}

    def __init__(self, capacity=4096):
        self._buf = (TraceRecord * capacity)()
        self.header = _TraceHeader(C.cast(self._buf, C.POINTER(TraceRecord)), capacity, 0)

    @property
    def count(self):
        return int(self.header.count)

    def records(self):
        k = min(self.count, int(self.header.capacity))
        return [(r.event, r.iterations, r.lambda_, r.residual, r.trial_residual, r.dx_dot) for r in self._buf[:k]]


class GpuOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("stream", C.c_void_p), ("comm", C.c_void_p),
                ("workspace", C.c_void_p), ("fbContext", C.c_void_p), ("fb", C.c_void_p), ("fd_batch", C.c_uint32),
                ("variant", C.c_uint32), ("stats", C.POINTER(Stats)), ("trace", C.POINTER(_TraceHeader)),
                ("fbRowMajor", C.c_void_p), ("fbRowMajorDiff", C.c_void_p), ("stats_size", C.c_uint32),
                ("reserved0", C.c_uint32)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(GpuOptions)
        self.stats_size = C.sizeof(Stats)


class BatchedOptions(C.Structure):
    """mir_lsq_batched_options: per-call options of the batched entries (variant bits, stream, caller-owned basis table,
    profiling buffer)."""
    _fields_ = [("struct_size", C.c_uint32), ("variant", C.c_uint32), ("stream", C.c_void_p), ("basis", C.c_void_p),
                ("basis_bytes", C.c_size_t), ("timing", C.c_void_p)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(BatchedOptions)


class BatchedExtras(C.Structure):
    """mir_lsq_batched_extras: per-row weights and the covariance output of the batched _ex entries."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("weights", C.c_void_p), ("weight_stride", C.c_size_t),
                ("covariance", C.c_void_p)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(BatchedExtras)


TASK_FN = C.CFUNCTYPE(None, _Task, C.c_uint32, C.c_uint32, C.c_uint32)
TM_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, _Task, TASK_FN)
ALLREDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


def _ftype(dtype):
    ct = C.c_double if dtype == np.float64 else C.c_float
    return C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(ct), C.POINTER(ct))


_lib = None
_wl = None


def _load(path):
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -m mir_optim_amd.build` "
                          "(hipcc --offload-arch=gfx950). mir_optim_amd has no CPU fallback.")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def lib():
    """The solver library (include/mir_optim_amd.h). Raises ImportError when it is not built."""
    global _lib
    if _lib is None:
        L = _load(_build.SOLVER_LIB)
        sz = C.c_size_t
        for name in ("mir_least_squares_work_length", "mir_least_squares_iwork_length"):
            getattr(L, name).restype = sz
            getattr(L, name).argtypes = [sz, sz]
        for name in ("mir_box_qp_work_length", "mir_box_qp_iwork_length"):
            getattr(L, name).restype = sz
            getattr(L, name).argtypes = [sz]
        L.mir_box_qp_iwork_length_ilp64.restype = sz
        L.mir_box_qp_iwork_length_ilp64.argtypes = [sz]
        L.mir_least_squares_iwork_length_ilp64.restype = sz
        L.mir_least_squares_iwork_length_ilp64.argtypes = [sz, sz]
        L.mir_least_squares_status_string.restype = C.c_char_p
        L.mir_least_squares_status_string.argtypes = [C.c_int]
        for suf, S, R in (("d", _Sd, _Rd), ("s", _Ss, _Rs)):
            getattr(L, "mir_least_squares_init_" + suf).argtypes = [C.POINTER(S)]
            getattr(L, "mir_least_squares_reset_" + suf).argtypes = [C.POINTER(S)]
            fn = getattr(L, "mir_optimize_least_squares_" + suf)
            fn.restype = R
            fn.argtypes = [C.POINTER(S), sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, _SliceD, _SliceD,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            fn = getattr(L, "mir_optimize_least_squares_gpu_" + suf)
            fn.restype = R
            fn.argtypes = [C.POINTER(S), sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GpuOptions),
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            fn = getattr(L, "mir_solve_box_qp_gpu_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                           C.POINTER(C.c_int)]
            fn = getattr(L, "mir_lsq_jtj_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.POINTER(C.c_float)]
            fn = getattr(L, "mir_lsq_covariance_gpu_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(S), sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GpuOptions),
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
            fn = getattr(L, "mir_lsq_spd_inverse_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            fn = getattr(L, "mir_lsq_spd_inverse_work_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, C.c_void_p]
        L.mir_lsq_spd_inverse_work_bytes.restype = sz
        L.mir_lsq_spd_inverse_work_bytes.argtypes = [sz, sz]
        L.mir_lsq_comm_create_local_group.restype = C.c_int
        L.mir_lsq_comm_create_local_group.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.mir_lsq_fd_diff_jtj_d.restype = C.c_int
        L.mir_lsq_fd_diff_jtj_d.argtypes = [sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(C.c_float)]
        L.mir_lsq_fd_jtj_d.restype = C.c_int
        L.mir_lsq_fd_jtj_d.argtypes = [sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
        L.mir_optimize_least_squares_batched_s.restype = C.c_int
        L.mir_optimize_least_squares_batched_s.argtypes = [C.POINTER(_Ss), sz, sz, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, sz, C.c_void_p, C.c_void_p, C.POINTER(BatchedOptions)]
        L.mir_lsq_batched_kernel_s.restype = C.c_int
        L.mir_lsq_batched_kernel_s.argtypes = [C.POINTER(_Ss), sz, sz, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, sz, C.c_void_p, C.c_void_p, C.POINTER(BatchedOptions)]
        L.mir_lsq_jtj_plan.restype = C.c_int
        L.mir_lsq_jtj_plan.argtypes = [sz, sz, sz, C.c_int, C.c_int, C.c_int, C.POINTER(sz * 10)]
        L.mir_lsq_selftest_reductions.restype = C.c_int
        L.mir_lsq_selftest_reductions.argtypes = [C.c_int, C.POINTER(C.c_int * 4)]
        for suf, S, ct in (("d", _Sd, C.c_double), ("s", _Ss, C.c_float)):
            fn = getattr(L, "mir_lsq_lm_solve_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(S), sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, ct,
                           C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int * 6)]
        L.mir_lsq_lm_solve_class.restype = C.c_int
        L.mir_lsq_lm_solve_class.argtypes = [sz, sz, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 3)]
        for suf, ct in (("d", C.c_double), ("s", C.c_float)):
            fn = getattr(L, "mir_lsq_lr_pass_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [sz, sz, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4 + [ct, ct] + [C.c_void_p] * 4 \
                + [C.POINTER(C.c_int * 6)]
            fn = getattr(L, "mir_lsq_lr_flush_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [sz, sz, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int * 2)]
        L.mir_lsq_lr_pass_scaled_d.restype = C.c_int
        L.mir_lsq_lr_pass_scaled_d.argtypes = [sz, sz, C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 4 \
            + [C.c_double, C.c_double] + [C.c_void_p] * 4 + [C.POINTER(C.c_int * 6)]
        L.mir_lsq_lr_flush_scaled_d.restype = C.c_int
        L.mir_lsq_lr_flush_scaled_d.argtypes = [sz, sz, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(C.c_int * 2)]
        L.mir_lsq_lr_class.restype = C.c_int
        L.mir_lsq_lr_class.argtypes = [sz, sz, C.c_int, C.POINTER(C.c_int * 2)]
        L.mir_lsq_lr_blocks.restype = C.c_int
        L.mir_lsq_lr_blocks.argtypes = [sz, C.c_int]
        vp, i2 = C.c_void_p, C.POINTER(C.c_int * 2)
        for suf, S, ct in (("d", _Sd, C.c_double), ("s", _Ss, C.c_float)):
            for name, args in (("decide", [C.POINTER(S), sz, C.c_int, C.c_uint, C.c_uint32, C.c_uint32] + [vp] * 8 + [C.c_int, C.c_int, vp, vp, i2]),
                               ("fd_points", [sz, vp, vp, vp, ct, C.c_int, vp, vp, vp, i2]),
                               ("fd_fill", [sz, sz, sz, C.c_int, C.c_int, vp, vp, vp, C.c_int, i2]),
                               ("entry_state", [sz, vp, C.c_uint32] + [vp] * 7 + [C.POINTER(C.c_int * 3)]),
                               ("unpack_grad", [sz, vp, vp, vp, vp, i2])):
                fn = getattr(L, "mir_lsq_%s_%s" % (name, suf))
                fn.restype, fn.argtypes = C.c_int, args
        L.mir_lsq_sumsq_blocks.restype = C.c_int
        L.mir_lsq_sumsq_blocks.argtypes = [sz]
        L.mir_lsq_batched_posvx_s.restype = C.c_int
        L.mir_lsq_batched_posvx_s.argtypes = [sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mir_optimize_least_squares_batched_d.restype = C.c_int
        L.mir_optimize_least_squares_batched_d.argtypes = [C.POINTER(_Sd), sz, sz, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, sz, C.c_void_p, C.c_void_p, C.POINTER(BatchedOptions)]
        L.mir_lsq_batched_kernel_d.restype = C.c_int
        L.mir_lsq_batched_kernel_d.argtypes = [C.POINTER(_Sd), sz, sz, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, sz, C.c_void_p, C.c_void_p, C.POINTER(BatchedOptions)]
        L.mir_lsq_batched_posvx_d.restype = C.c_int
        L.mir_lsq_batched_posvx_d.argtypes = [sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for suf, S in (("s", _Ss), ("d", _Sd)):
            for name in ("mir_optimize_least_squares_batched_ex_", "mir_lsq_batched_kernel_ex_", "mir_lsq_batched_covariance_"):
                fn = getattr(L, name + suf)
                fn.restype = C.c_int
                fn.argtypes = [C.POINTER(S), sz, sz, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, C.c_void_p,
                               C.c_void_p, C.POINTER(BatchedOptions), C.POINTER(BatchedExtras)]
        for name in ("mir_optimize_least_squares_batched16_d", "mir_lsq_batched16_kernel_d", "mir_optimize_least_squares_batched16_ex_d",
                     "mir_lsq_batched16_kernel_ex_d", "mir_lsq_batched16_covariance_d"):
            fn = getattr(L, name)
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(_Sd), sz, sz, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, C.c_void_p,
                           C.c_void_p, C.POINTER(BatchedOptions), C.POINTER(BatchedExtras)]
        for name, S in (("mir_lsq_batched_predict_s", _Ss), ("mir_lsq_batched_predict_d", _Sd), ("mir_lsq_batched16_predict_d", _Sd)):
            fn = getattr(L, name)
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(S), sz, sz, C.c_int] + [C.c_void_p] * 4 + [sz] + [C.c_void_p] * 3 \
                + [C.POINTER(BatchedOptions), C.POINTER(BatchedExtras)]
        L.mir_lsq_batched16_jtj_d.restype = C.c_int
        L.mir_lsq_batched16_jtj_d.argtypes = [sz, sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("box_qp_s", "box_qp_d", "box_qp16_s", "box_qp16_d"):
            fn = getattr(L, "mir_lsq_batched_" + name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_uint, C.c_void_p]
        for name in ("box_qp64_s", "box_qp64_d", "box_qp64_waves_s", "box_qp64_waves_d"):
            fn = getattr(L, "mir_lsq_batched_" + name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_uint, C.c_void_p] + ([C.c_uint] if "waves" in name else [])
        for suf in ("s", "d"):
            fn = getattr(L, "mir_lsq_batched_posvx16_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [sz, sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mir_lsq_comm_describe.restype = C.c_int
        L.mir_lsq_comm_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.mir_lsq_workspace_create.restype = C.c_void_p
        L.mir_lsq_workspace_create.argtypes = [sz, sz, sz]
        L.mir_lsq_workspace_destroy.argtypes = [C.c_void_p]
        L.mir_lsq_rccl_unique_id.restype = C.c_int
        L.mir_lsq_rccl_unique_id.argtypes = [C.c_void_p]
        L.mir_lsq_comm_create_rccl.restype = C.c_void_p
        L.mir_lsq_comm_create_rccl.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.mir_lsq_comm_create_callback.restype = C.c_void_p
        L.mir_lsq_comm_create_callback.argtypes = [C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]
        L.mir_lsq_comm_destroy.argtypes = [C.c_void_p]
        L.mir_lsq_comm_record.restype = C.c_int
        L.mir_lsq_comm_record.argtypes = [C.c_void_p, C.c_void_p, sz]
        L.mir_lsq_comm_recorded.restype = sz
        L.mir_lsq_comm_recorded.argtypes = [C.c_void_p]
        L.mir_lsq_comm_create_replay.restype = C.c_void_p
        L.mir_lsq_comm_create_replay.argtypes = [C.c_int, C.c_int, C.c_void_p, sz, C.c_void_p]
        L.mir_lsq_comm_replay_rewind.restype = C.c_int
        L.mir_lsq_comm_replay_rewind.argtypes = [C.c_void_p]
        L.mir_lsq_comm_replay_set_delay.restype = C.c_int
        L.mir_lsq_comm_replay_set_delay.argtypes = [C.c_void_p, C.c_uint]
        L.mir_lsq_comm_ranks.restype = C.c_int
        L.mir_lsq_comm_ranks.argtypes = [C.c_void_p]
        for name in ("mir_lsq_comm_allreduce_d", "mir_lsq_comm_allreduce_s"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, sz, C.c_void_p]
        L.mir_lsq_device_count.restype = C.c_int
        L.mir_lsq_device_malloc.restype = C.c_void_p
        L.mir_lsq_device_malloc.argtypes = [sz]
        L.mir_lsq_device_free.argtypes = [C.c_void_p]
        for name in ("mir_lsq_memcpy_h2d", "mir_lsq_memcpy_d2h", "mir_lsq_memcpy_d2d"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, sz, C.c_void_p]
        L.mir_lsq_stream_create.restype = C.c_void_p
        L.mir_lsq_stream_destroy.argtypes = [C.c_void_p]
        L.mir_lsq_stream_synchronize.restype = C.c_int
        L.mir_lsq_stream_synchronize.argtypes = [C.c_void_p]
        L.mir_lsq_version.restype = C.c_char_p
        for suf, S, R, ct in (("d", _Sd, _Rd, C.c_double), ("s", _Ss, _Rs, C.c_float)):
            fn = getattr(L, "mir_fit_spline_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(S), sz, C.c_void_p, sz, C.c_void_p, C.c_void_p, C.c_void_p, ct, C.c_void_p,
                           C.c_void_p, C.c_void_p, C.POINTER(R)]
            getattr(L, "mir_spline_c2_derivatives_" + suf).argtypes = [sz, C.c_void_p, C.c_void_p, C.c_void_p]
            getattr(L, "mir_spline_eval_" + suf).argtypes = [sz, C.c_void_p, C.c_void_p, C.c_void_p, ct, C.c_void_p]
        L.mir_fit_spline_residuals_d.argtypes = [sz, C.c_void_p, sz, C.c_void_p, C.c_double, C.c_void_p, sz, C.c_void_p]
        for suf, S, R, ct in (("d", _Sd, _Rd, C.c_double), ("s", _Ss, _Rs, C.c_float)):
            fn = getattr(L, "mir_fit_spline_gpu_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(S), sz, C.c_void_p, sz, C.c_void_p, C.c_void_p, C.c_void_p, ct, C.POINTER(GpuOptions),
                           C.c_void_p, C.c_void_p, C.POINTER(R)]
            fn = getattr(L, "mir_spline_eval_gpu_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [sz, C.c_void_p, C.c_void_p, C.c_void_p, sz, C.c_void_p, C.c_void_p, C.c_void_p]
            for name in ("mir_fit_spline_gpu_eval_", "mir_fit_spline_eval_host_"):
                fn = getattr(L, name + suf)
                fn.restype = C.c_int
                fn.argtypes = [sz, C.c_void_p, sz, C.c_void_p, ct, sz, C.c_void_p, C.c_int, C.c_void_p]
            fn = getattr(L, "mir_fit_spline_factor_" + suf)
            fn.restype = C.c_int
            fn.argtypes = [sz, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def workloads_lib():
    """Device residual callbacks of the synthetic workloads (csrc/workloads.hip)."""
    global _wl
    if _wl is None:
        W = _load(_build.WORKLOADS_LIB)
        W.wl_uniform.argtypes = [C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p]
        W.wl_tanh_linear_generate.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        sz = C.c_size_t
        W.wl_tanh_linear_class.restype = C.c_int
        W.wl_tanh_linear_class.argtypes = [C.c_int, sz, sz, sz, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 4)]
        W.wl_gauss_sum_class.restype = C.c_int
        W.wl_gauss_sum_class.argtypes = [C.c_int, sz, sz, sz, C.POINTER(C.c_int * 2)]
        for name in ("wl_unary_d", "wl_unary_s"):
            getattr(W, name).restype = C.c_int
            getattr(W, name).argtypes = [C.c_void_p, C.c_int, sz, C.c_void_p, C.c_void_p]
        _wl = W
    return _wl


def device_count():
    return lib().mir_lsq_device_count()


def leastSquaresStatusString(st):
    return lib().mir_least_squares_status_string(int(st)).decode()


def mir_least_squares_work_length(m, n):
    return lib().mir_least_squares_work_length(m, n)


def mir_least_squares_iwork_length(m, n):
    return lib().mir_least_squares_iwork_length(m, n)


def mir_box_qp_work_length(n):
    return lib().mir_box_qp_work_length(n)


def mir_box_qp_iwork_length(n):
    return lib().mir_box_qp_iwork_length(n)


def LeastSquaresSettings(dtype=np.float64):
    """LeastSquaresSettings!T with the reference defaults (LS:93-122) written by mir_least_squares_init_*."""
    s = _Sd() if dtype == np.float64 else _Ss()
    (lib().mir_least_squares_init_d if dtype == np.float64 else lib().mir_least_squares_init_s)(C.byref(s))
    return s


def BoxQPSettings(dtype=np.float64):
    return LeastSquaresSettings(dtype).qpSettings


class LeastSquaresResult:
    """LeastSquaresResult!T (LS:128-143)."""

    def __init__(self, raw):
        self.status = LeastSquaresStatus(raw.status)
        self.iterations = raw.iterations
        self.fCalls = raw.fCalls
        self.gCalls = raw.gCalls
        self.residual = raw.residual
        self.lambda_ = raw.lambda_

    def __repr__(self):
        return (f"LeastSquaresResult(status={self.status.name}, iterations={self.iterations}, fCalls={self.fCalls}, "
                f"gCalls={self.gCalls}, residual={self.residual!r}, lambda={self.lambda_!r})")


class Stream:
    def __init__(self):
        self.handle = lib().mir_lsq_stream_create()
        if not self.handle:
            raise RuntimeError("hipStreamCreate failed (no GPU?)")

    def synchronize(self):
        if lib().mir_lsq_stream_synchronize(self.handle) != 0:
            raise RuntimeError("stream synchronize failed")

    def close(self):
        if self.handle:
            lib().mir_lsq_stream_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """A device allocation filled from / read back to numpy (plumbing for tests and the bench)."""

    def __init__(self, array=None, nbytes=None, dtype=None, shape=None):
        if array is not None:
            array = np.ascontiguousarray(array)
            nbytes, dtype, shape = array.nbytes, array.dtype, array.shape
        self.nbytes, self.dtype, self.shape = int(nbytes), np.dtype(dtype), tuple(shape)
        self.ptr = lib().mir_lsq_device_malloc(max(self.nbytes, 8))
        if not self.ptr:
            raise MemoryError(f"hipMalloc({self.nbytes}) failed (no GPU?)")
        if array is not None:
            self.upload(array)

    def upload(self, array):
        array = np.ascontiguousarray(array, dtype=self.dtype)
        assert array.nbytes == self.nbytes
        if lib().mir_lsq_memcpy_h2d(self.ptr, array.ctypes.data, self.nbytes, None) != 0:
            raise RuntimeError("H2D copy failed")

    def upload_at(self, byte_offset, array):
        """Copy `array` into the allocation at `byte_offset` (building a large device array piece by piece)."""
        array = np.ascontiguousarray(array, dtype=self.dtype)
        assert 0 <= byte_offset and byte_offset + array.nbytes <= self.nbytes
        if lib().mir_lsq_memcpy_h2d(self.ptr + byte_offset, array.ctypes.data, array.nbytes, None) != 0:
            raise RuntimeError("H2D copy failed")

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if lib().mir_lsq_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes, None) != 0:
            raise RuntimeError("D2H copy failed")
        return out

    def free(self):
        if self.ptr:
            lib().mir_lsq_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _as_fnptr(cb, ftype, wrap, keep):
    if cb is None:
        return C.c_void_p(None)
    if callable(cb):
        c = ftype(wrap(cb))
        keep.append(c)
        return C.cast(c, C.c_void_p)
    return C.c_void_p(int(cb))


def _wrap_callbacks(f, g, tm, dtype):
    """The C function pointers of f, g and tm for a call (python callables are wrapped, integer addresses passed through).
    Returns (fptr, gptr, tmptr, keep, errors): `keep` holds the ctypes thunks alive for the duration of the call, `errors`
    collects what the python callbacks raised."""
    ft = _ftype(dtype)
    keep = []
    errors = []      # exceptions raised inside Python callbacks: ctypes would print and swallow them and the solve would go
                     # on with garbage -- they are recorded, the outputs poisoned with NaN (the solver then ends with
                     # numericError at its next check, LS:990 / 1117) and the first one is re-raised after the C call returns

    def wrap_f(fn):
        def cb(_ctx, m_, n_, xp, yp):
            yv = np.ctypeslib.as_array(yp, shape=(m_,))
            try:
                xv = np.ctypeslib.as_array(xp, shape=(n_,))
                yv[:] = 0
                fn(xv, yv)
            except BaseException as e:      # noqa: BLE001 -- re-raised below
                errors.append(e)
                yv[:] = np.nan
        return cb

    def wrap_g(fn):
        def cb(_ctx, m_, n_, xp, Jp):
            Jv = np.ctypeslib.as_array(Jp, shape=(m_ * n_,)).reshape(m_, n_)
            try:
                xv = np.ctypeslib.as_array(xp, shape=(n_,))
                Jv[:] = 0
                fn(xv, Jv)
            except BaseException as e:      # noqa: BLE001
                errors.append(e)
                Jv[:] = np.nan
        return cb

    fptr = _as_fnptr(f, ft, wrap_f, keep)
    gptr = _as_fnptr(g, ft, wrap_g, keep)
    tmptr = C.c_void_p(None)
    if tm is not None:
        def tm_cb(_ctx, count, task, taskfn):
            try:
                tm(count, lambda total, tid, i: taskfn(task, total, tid, i))
            except BaseException as e:      # noqa: BLE001
                errors.append(e)
        tmc = TM_FN(tm_cb)
        keep.append(tmc)
        tmptr = C.cast(tmc, C.c_void_p)
    return fptr, gptr, tmptr, keep, errors


def optimizeLeastSquares(f, m, x, l=None, u=None, g=None, tm=None, settings=None, dtype=np.float64,
                         fContext=None, gContext=None, options=None, gpu_entry=None):
    """High level nothrow API (LS:459-519). `x` is updated in place (numpy array) and returned with the result.

    f, g : python callables f(x, y) / g(x, J) working on numpy views of HOST memory (y and J are
           zero-filled before the call like the template tier does, LS:469, LS:482), or integer
           addresses of native callbacks (then fContext / gContext are passed through).
    tm   : optional python thread manager tm(count, task) where task(totalThreads, threadId, i)
           must be called for every i in [0, count) (LS:575-578).
    options : GpuOptions for the additive entry point (device callbacks, comm, stats, ...)."""
    L = lib()
    dbl = dtype == np.float64
    x = np.ascontiguousarray(x, dtype=dtype)
    n = x.size
    lo = np.full(n, -np.inf, dtype=dtype) if l is None else np.ascontiguousarray(l, dtype=dtype)
    up = np.full(n, np.inf, dtype=dtype) if u is None else np.ascontiguousarray(u, dtype=dtype)
    if settings is None:
        settings = LeastSquaresSettings(dtype)
    fptr, gptr, tmptr, keep, errors = _wrap_callbacks(f, g, tm, dtype)
    use_gpu_entry = gpu_entry if gpu_entry is not None else (options is not None)
    suf = "d" if dbl else "s"
    if use_gpu_entry:
        fn = getattr(L, "mir_optimize_least_squares_gpu_" + suf)
        raw = fn(C.byref(settings), m, n, x.ctypes.data, lo.ctypes.data, up.ctypes.data,
                 C.byref(options) if options is not None else None, fContext, fptr, gContext, gptr, None, tmptr)
    else:
        # the reference's own entry point (LS:705-724): work / iwork are sized by the reference formulas
        wl = L.mir_least_squares_work_length(m, n)
        iwl = L.mir_least_squares_iwork_length(m, n)
        iwork = np.zeros(iwl + 4, dtype=np.int32)
        work_slice = _SliceD(wl, None)      # never dereferenced by this implementation
        iwork_slice = _SliceD(iwl, iwork.ctypes.data)
        fn = getattr(L, "mir_optimize_least_squares_" + suf)
        raw = fn(C.byref(settings), m, n, x.ctypes.data, lo.ctypes.data, up.ctypes.data, work_slice, iwork_slice,
                 fContext, fptr, gContext, gptr, None, tmptr)
    del keep
    if errors:
        raise errors[0]
    return LeastSquaresResult(raw), x


def optimize(f, m, x, l=None, u=None, g=None, tm=None, settings=None, dtype=np.float64, taskPool=None, **kw):
    """High level throwing API (LS:165-215): raises LeastSquaresException when status < 0.

    taskPool: optional concurrent.futures-like executor with `_max_workers`; mirrors the task-pool
    overload LS:184-215 (finite-difference columns are evaluated by the pool's threads)."""
    if taskPool is not None and tm is None:
        import threading
        workers = max(1, getattr(taskPool, "_max_workers", 1))
        ids = {}
        lock = threading.Lock()

        def tm(count, task):
            def run(i):
                with lock:
                    tid = ids.setdefault(threading.get_ident(), len(ids))
                task(workers, tid % workers, i)
            list(taskPool.map(run, range(count)))
    res, xo = optimizeLeastSquares(f, m, x, l, u, g, tm, settings, dtype, **kw)
    if res.status < 0:
        raise LeastSquaresException(res.status, res)
    return res, xo


def _batched_suffix(dtype):
    """'s' for float32 (the default of the batched entries), 'd' for float64"""
    if np.dtype(dtype) == np.float32:
        return "s"
    if np.dtype(dtype) == np.float64:
        return "d"
    raise ValueError(f"the batched entries exist in float32 and float64, not {np.dtype(dtype)}")


def _batched_bounds(l, u, count, n, dtype):
    """l / u of a batched call as contiguous arrays of `dtype`: (lo, up, per_problem). Each is None, n values (one box for the
    batch) or count x n (row k the box of problem k); the two have one shape, a None takes its partner's (-inf / +inf)."""
    lo = None if l is None else np.ascontiguousarray(l, dtype=dtype)
    up = None if u is None else np.ascontiguousarray(u, dtype=dtype)
    shape = lo.shape if lo is not None else up.shape if up is not None else (n,)
    if shape not in ((n,), (count, n)) or (up is not None and up.shape != shape):
        raise ValueError(f"l and u: {n} values each or {count} x {n} each, not {None if lo is None else lo.shape} and "
                         f"{None if up is None else up.shape}")
    if lo is None:
        lo = np.full(shape, -np.inf, dtype=dtype)
    if up is None:
        up = np.full(shape, np.inf, dtype=dtype)
    return lo, up, len(shape) == 2


def optimizeLeastSquaresBatched(model, x, t, data, l=None, u=None, settings=None, variant=0, dtype=np.float32, weights=None,
                                covariance=False, absolute_sigma=False):
    """Many independent small fits, one wavefront per problem (mir_optimize_least_squares_batched_s, fp32, or with
    dtype=np.float64 mir_optimize_least_squares_batched_d). x: count x n starts (a copy is updated and returned), t: m
    (shared) or count x m, data: count x m. variant: BATCHED_* bits (per call). Returns (list of LeastSquaresResult, x).
    weights: m (shared) or count x m values w_i = 1 / sigma_i; the residual of row i becomes w_i (model - data_i), a weight of 0
    removes the row. covariance=True: returns (results, x, cov), cov count x n x n = s^2 inv(J^T J) at the returned x with
    s^2 = residual / (rows with nonzero weight - n), or s^2 = 1 with absolute_sigma=True; +inf for a singular J^T J or no
    degrees of freedom, NaN for a problem with a negative status. Any of the three goes through the _ex entry
    (mir_optimize_least_squares_batched_ex_s / _d); a call without them is the call it always was.
    l / u: n values (one box for the batch) or count x n (row k is the box of problem k; a None beside a 2-D partner is -inf /
    +inf of that shape; anything else raises ValueError). 2-D bounds go through the _ex entry with BATCHED_BOUNDS_PER_PROBLEM;
    1-D bounds make the call they always made. A parameter with l_j == u_j is fixed: the fit keeps it there, and its row and
    column of the covariance are 0 (s^2 then divides by rows - the number of free parameters).
    A MODEL16_* id (9 to 16 parameters) goes to mir_optimize_least_squares_batched16_d: dtype must be float64, and weights,
    covariance and absolute_sigma raise ValueError (optimizeLeastSquaresBatched16 takes them)."""
    if int(model) in _MODELS16:
        return _optimize_batched16(model, x, t, data, l, u, settings, variant, dtype, weights, covariance, absolute_sigma)
    suf = _batched_suffix(dtype)
    p = _batched_pack(x, t, data, l, u, settings, np.float32 if suf == "s" else np.float64)
    if weights is None and not covariance and not absolute_sigma and not p.per_problem:
        return _batched_call("mir_optimize_least_squares_batched_" + suf, model, p, variant)        # no extras argument: the old entry
    ex, cov = _batched_extras(p, weights, covariance, absolute_sigma)
    return _batched_call("mir_optimize_least_squares_batched_ex_" + suf, model, p, variant, C.byref(ex), cov=cov)


def _batched_pack(x, t, data, l, u, settings, dtype, check_shapes=False):
    """The arguments of a batched call as the C entries take them: x (a copy), t, data and the bounds as contiguous arrays of
    `dtype`, the settings and the result records. check_shapes: x, data and t must agree (ValueError)."""
    x = np.array(x, dtype=dtype, order="C")
    data = np.ascontiguousarray(data, dtype=dtype)
    t = np.ascontiguousarray(t, dtype=dtype)
    if check_shapes and (x.ndim != 2 or data.ndim != 2 or data.shape[0] != x.shape[0]):
        raise ValueError(f"x: count x n and data: count x m, not {x.shape} and {data.shape}")
    count, n = x.shape
    m = data.shape[1]
    if check_shapes and t.shape not in ((m,), (count, m)):
        raise ValueError(f"t: {m} values or {count} x {m}, not {t.shape}")
    lo, up, per_problem = _batched_bounds(l, u, count, n, dtype)
    return types.SimpleNamespace(dtype=dtype, x=x, t=t, data=data, count=count, n=n, m=m, t_stride=0 if t.ndim == 1 else m, lo=lo, up=up,
                                 per_problem=per_problem, settings=LeastSquaresSettings(dtype) if settings is None else settings,
                                 raw=((_Rs if dtype == np.float32 else _Rd) * count)())


def _batched_extras(p, weights, covariance, absolute_sigma):
    """(BatchedExtras, cov) of a packed call: the flags, the weights (m values or count x m) and the covariance to fill, or None.
    The extras keep their arrays alive."""
    ex = BatchedExtras(flags=(BATCHED_ABSOLUTE_SIGMA if absolute_sigma else 0) | (BATCHED_BOUNDS_PER_PROBLEM if p.per_problem else 0))
    if weights is not None:
        ex._weights = weights = np.ascontiguousarray(weights, dtype=p.dtype)
        if weights.shape not in ((p.m,), (p.count, p.m)):
            raise ValueError(f"weights: {p.m} values or {p.count} x {p.m}, not {weights.shape}")
        ex.weights = weights.ctypes.data
        ex.weight_stride = 0 if weights.ndim == 1 else p.m
    cov = np.empty((p.count, p.n, p.n), dtype=p.dtype) if covariance else None
    if covariance:
        ex.covariance = cov.ctypes.data
    return ex, cov


def _batched_call(name, model, p, variant, *extras, cov=None):
    """Calls the host-pointer entry `name` on a packed call. extras: nothing for an entry without that argument, else the argument
    (None: a null pointer); cov: the array its covariance points to. Returns (results, x), with cov (results, x, cov)."""
    rc = getattr(lib(), name)(C.byref(p.settings), p.count, p.m, int(model), p.x.ctypes.data, p.lo.ctypes.data, p.up.ctypes.data,
                              p.t.ctypes.data, p.t_stride, p.data.ctypes.data, p.raw, C.byref(BatchedOptions(variant=variant)), *extras)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {rc}")
    res = [LeastSquaresResult(r) for r in p.raw]
    return (res, p.x) if cov is None else (res, p.x, cov)


def _optimize_batched16(model, x, t, data, l, u, settings, variant, dtype, weights, covariance, absolute_sigma):
    """optimizeLeastSquaresBatched for a MODEL16_* id"""
    if np.dtype(dtype) != np.float64:
        raise ValueError(f"the MODEL16_* models are fitted in float64 only, not {np.dtype(dtype)}: pass dtype=np.float64")
    if weights is not None or covariance or absolute_sigma:
        raise ValueError("the MODEL16_* models take neither weights nor covariance here: call optimizeLeastSquaresBatched16")
    p = _batched_pack(x, t, data, l, u, settings, np.float64)
    # 2-D bounds: this entry with an extras that carries the flag and nothing else; 1-D: no extras, as always
    ex = BatchedExtras(flags=BATCHED_BOUNDS_PER_PROBLEM) if p.per_problem else None
    return _batched_call("mir_optimize_least_squares_batched16_d", model, p, variant, C.byref(ex) if p.per_problem else None)


def optimizeLeastSquaresBatched16(model, x, t, data, l=None, u=None, settings=None, variant=0, weights=None, covariance=False,
                                  absolute_sigma=False):
    """Many independent fits of a MODEL16_* model (9 to 16 parameters, float64 only), one wavefront per problem, with per-row
    weights and the covariance of the fitted parameters (mir_optimize_least_squares_batched16_ex_d). x: count x n starts (a copy
    is updated and returned), t: m (shared) or count x m, data: count x m, m <= 1119. weights: m (shared) or count x m values
    w_i = 1 / sigma_i; the residual of row i becomes w_i (model - data_i), a weight of 0 removes the row (problems of different
    lengths are padded to a common m that way). covariance=True: returns (results, x, cov), cov count x n x n =
    s^2 inv(J^T J) at the returned x with s^2 = residual / (rows with nonzero weight - n), or s^2 = 1 with absolute_sigma=True;
    +inf for a singular J^T J or no degrees of freedom, NaN for a problem with a negative status. Otherwise returns (results, x).
    A call with none of the three is the call optimizeLeastSquaresBatched makes for these models.
    l / u: n values or count x n (row k the box of problem k), as in optimizeLeastSquaresBatched; l_j == u_j fixes parameter j."""
    if int(model) not in _MODELS16:
        raise ValueError(f"optimizeLeastSquaresBatched16 takes a MODEL16_* id, not {model}")
    for name, a in (("x", x), ("t", t), ("data", data), ("weights", weights)):
        dt = getattr(a, "dtype", None)
        if dt is not None and np.issubdtype(dt, np.floating) and dt != np.float64:
            raise ValueError(f"the MODEL16_* models are fitted in float64 only: {name} is {dt}")
    if weights is None and not covariance and not absolute_sigma:
        return _optimize_batched16(model, x, t, data, l, u, settings, variant, np.float64, None, False, False)
    p = _batched_pack(x, t, data, l, u, settings, np.float64, check_shapes=True)
    ex, cov = _batched_extras(p, weights, covariance, absolute_sigma)
    return _batched_call("mir_optimize_least_squares_batched16_ex_d", model, p, variant, C.byref(ex), cov=cov)


def batched16JtJ(J, y):
    """The J^T J stage of the 9 .. 16 parameter batched kernel on its own (mir_lsq_batched16_jtj_d): J count x m x n (n <= 16),
    y count x m. Returns (JJ count x 16 x 16, Jy count x 16)."""
    L = lib()
    J = np.ascontiguousarray(J, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    count, m, n = J.shape
    dJ, dy = DeviceBuffer(J), DeviceBuffer(y)
    dJJ = DeviceBuffer(nbytes=count * 256 * 8, dtype=np.float64, shape=(count, 16, 16))
    dJy = DeviceBuffer(nbytes=count * 16 * 8, dtype=np.float64, shape=(count, 16))
    st = Stream()
    rc = L.mir_lsq_batched16_jtj_d(count, m, n, dJ.ptr, dy.ptr, dJJ.ptr, dJy.ptr, st.handle)
    if rc != 0:
        raise RuntimeError(f"mir_lsq_batched16_jtj_d failed: {rc}")
    st.synchronize()
    JJ, Jy = dJJ.download().copy(), dJy.download().copy()
    for b in (dJ, dy, dJJ, dJy):
        b.free()
    return JJ, Jy


BATCHED_NO_LADDER = 1
BATCHED_ANALYTIC_JACOBIAN = 2   # MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN: the model's own derivative instead of finite differences
BATCHED_DEVICE_BOUNDS = 4       # MIR_LSQ_BATCHED_DEVICE_BOUNDS: bounded steps are solved inside the wave kernel (no -100, no fallback)
BATCHED_ABSOLUTE_SIGMA = 1      # mir_lsq_batched_extras.flags
BATCHED_BOUNDS_PER_PROBLEM = 2  # mir_lsq_batched_extras.flags: lower / upper hold count x n values, row k the box of problem k


def batchedPosvx(P, rhs, dtype=np.float32):
    """The damped solve of the wave-per-problem kernel on its own (mir_lsq_batched_posvx_s, or with dtype=np.float64
    mir_lsq_batched_posvx_d): P count x n x n (lower triangles read), rhs count x n, n in (3, 8). Returns (x count x n,
    info count). n = 9 .. 16 goes to the 16-row solve of the batched box-constrained QPs in its 16-wide layout
    (mir_lsq_batched_posvx16_s / _d)."""
    suf = _batched_suffix(dtype)
    dtype = np.float32 if suf == "s" else np.float64
    L = lib()
    P = np.asarray(P, dtype=dtype)
    count, n = P.shape[0], P.shape[1]
    w, name = (8, "mir_lsq_batched_posvx_" + suf) if n <= 8 else (16, "mir_lsq_batched_posvx16_" + suf)
    Pp = np.zeros((count, w, w), dtype=dtype); Pp[:, :n, :n] = P
    bp = np.zeros((count, w), dtype=dtype); bp[:, :n] = rhs
    dP, db = DeviceBuffer(Pp), DeviceBuffer(bp)
    dx = DeviceBuffer(nbytes=count * w * np.dtype(dtype).itemsize, dtype=dtype, shape=(count, w))
    di = DeviceBuffer(nbytes=count * 4, dtype=np.int32, shape=(count,))
    st = Stream()
    rc = getattr(L, name)(count, n, dP.ptr, db.ptr, dx.ptr, di.ptr, st.handle)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {rc}")
    st.synchronize()
    x, info = dx.download()[:, :n].copy(), di.download().copy()
    for b in (dP, db, dx, di):
        b.free()
    return x, info


_MODEL_N = {MODEL_EXP_DECAY: 3, MODEL_EXP3_AFFINE: 8, MODEL_EXP_DECAY_PAD8: 8, MODEL16_EXP_HARM16: 16, MODEL16_GAUSS3_AFFINE: 11}


def predictBatched(model, x, tq, covariance=None, l=None, u=None, settings=None, variant=0, dtype=np.float32):
    """The fitted curve of every problem of a batch on a grid of abscissae, and its 1-sigma confidence band
    (mir_lsq_batched_predict_s, with dtype=np.float64 mir_lsq_batched_predict_d; a MODEL16_* id goes to
    mir_lsq_batched16_predict_d and requires float64). x: count x n fitted parameters; tq: q abscissae for all problems or
    count x q. Returns value (count x q) = model(tq; x_k) -- or, with covariance (count x n x n, as a batched fit with
    covariance=True returns it), (value, sigma): sigma = sqrt(g^T C_k g), g the derivative of the model with respect to its
    parameters at tq, by central differences with settings.jacobianEpsilon clipped to l / u (variant=BATCHED_ANALYTIC_JACOBIAN:
    the model's own derivative, for a model that has one). l / u: None, n values or count x n, as in
    optimizeLeastSquaresBatched; a parameter with l_j == u_j is fixed and contributes nothing to the band. sigma is +inf where
    the covariance is (a degenerate problem) and NaN where the fit had failed; value is computed for every problem.
    Wrong shapes raise ValueError."""
    model = int(model)
    wide = model in _MODELS16
    if wide and np.dtype(dtype) != np.float64:
        raise ValueError(f"the MODEL16_* models are evaluated in float64 only, not {np.dtype(dtype)}: pass dtype=np.float64")
    suf = _batched_suffix(dtype)
    dtype = np.float32 if suf == "s" else np.float64
    x = np.ascontiguousarray(x, dtype=dtype)
    tq = np.ascontiguousarray(tq, dtype=dtype)
    if x.ndim != 2 or (model in _MODEL_N and x.shape[1] != _MODEL_N[model]):
        raise ValueError(f"x: count x n{' with n = %d' % _MODEL_N[model] if model in _MODEL_N else ''}, not {x.shape}")
    count, n = x.shape
    if tq.ndim not in (1, 2) or (tq.ndim == 2 and tq.shape[0] != count):
        raise ValueError(f"tq: q values or {count} x q, not {tq.shape}")
    q = tq.shape[-1]
    if covariance is not None:
        covariance = np.ascontiguousarray(covariance, dtype=dtype)
        if covariance.shape != (count, n, n):
            raise ValueError(f"covariance: {count} x {n} x {n}, not {covariance.shape}")
    bounded = l is not None or u is not None
    lo, up, per_problem = _batched_bounds(l, u, count, n, dtype) if bounded else (None, None, False)
    S = LeastSquaresSettings(dtype) if settings is None else settings
    value = np.empty((count, q), dtype=dtype)
    if count == 0 or q == 0:
        return value if covariance is None else (value, np.empty((count, q), dtype=dtype))
    ins = [DeviceBuffer(a) if a is not None else None for a in (x, lo, up, tq, covariance)]
    outs = [DeviceBuffer(nbytes=value.nbytes, dtype=dtype, shape=value.shape) for _ in range(1 if covariance is None else 2)]
    ptr = [b.ptr if b is not None else None for b in ins]
    st = Stream()
    name = "mir_lsq_batched16_predict_d" if wide else "mir_lsq_batched_predict_" + suf
    ex = BatchedExtras(flags=BATCHED_BOUNDS_PER_PROBLEM if per_problem else 0)
    rc = getattr(lib(), name)(C.byref(S), count, q, model, ptr[0], ptr[1], ptr[2], ptr[3], 0 if tq.ndim == 1 else q, ptr[4], outs[0].ptr,
                              outs[1].ptr if len(outs) == 2 else None, C.byref(BatchedOptions(variant=variant, stream=st.handle)),
                              C.byref(ex))
    if rc != 0:
        raise RuntimeError(f"{name} failed: {rc}")
    st.synchronize()
    res = [b.download().copy() for b in outs]
    for b in ins + outs:
        if b is not None:
            b.free()
    return res[0] if covariance is None else (res[0], res[1])


COVARIANCE_ABSOLUTE_SIGMA = 1      # MIR_LSQ_COVARIANCE_ABSOLUTE_SIGMA


def covariance(f, m, x, l=None, u=None, g=None, tm=None, settings=None, dtype=np.float64, absolute_sigma=False,
               fContext=None, gContext=None, options=None):
    """Covariance of the fitted parameters of the general solver at x (mir_lsq_covariance_gpu_*): cov = s^2 inv(J^T J) from one
    full Jacobian refresh made as the solve makes it (g, or finite differences through f / the options' batched callbacks), with
    s^2 = ||f(x)||^2 / (rows - free parameters), or 1 with absolute_sigma=True. f, g, tm, fContext, gContext and options as in
    optimizeLeastSquares (device callbacks, workspace, communicator, stats). x is not modified. A parameter with l == u is
    fixed: its row and column are 0. Returns (cov n x n, stderr = sqrt(diag(cov)), residual ||f(x)||^2, info); info != 0: J^T J
    is not positive definite at that leading minor and the free entries are +inf. Raises LeastSquaresException for a negative
    status (bad guess, bad bounds, bad settings, no device)."""
    L = lib()
    x = np.array(x, dtype=dtype, order="C")
    n = x.size
    lo = np.full(n, -np.inf, dtype=dtype) if l is None else np.ascontiguousarray(l, dtype=dtype)
    up = np.full(n, np.inf, dtype=dtype) if u is None else np.ascontiguousarray(u, dtype=dtype)
    if settings is None:
        settings = LeastSquaresSettings(dtype)
    fptr, gptr, tmptr, keep, errors = _wrap_callbacks(f, g, tm, dtype)
    cov = np.empty((n, n), dtype=dtype)
    res = np.zeros(1, dtype=dtype)
    info = C.c_int(0)
    fn = getattr(L, "mir_lsq_covariance_gpu_" + ("d" if dtype == np.float64 else "s"))
    rc = fn(C.byref(settings), m, n, x.ctypes.data, lo.ctypes.data, up.ctypes.data,
            C.byref(options) if options is not None else None, fContext, fptr, gContext, gptr, None, tmptr,
            COVARIANCE_ABSOLUTE_SIGMA if absolute_sigma else 0, cov.ctypes.data, res.ctypes.data, C.byref(info))
    del keep
    if errors:
        raise errors[0]
    if rc == -1:
        raise ValueError("mir_lsq_covariance_gpu: NULL argument")
    if rc != 0:
        raise LeastSquaresException(rc)
    with np.errstate(invalid="ignore"):
        stderr = np.sqrt(np.diag(cov))
    return cov, stderr, res[0], info.value


def spdInverse(P, fixed=None, dtype=np.float64):
    """The inverse of a symmetric positive definite matrix on the device (mir_lsq_spd_inverse_*): P n x n (lower triangle
    read), fixed: n flags or None -- a fixed index is taken out of the system and its row and column are 0. Returns (X, info);
    info != 0: the leading minor of that order among the free indices is not positive, the free entries of X are +inf."""
    suf = _batched_suffix(dtype)
    dtype = np.float32 if suf == "s" else np.float64
    L = lib()
    P = np.ascontiguousarray(P, dtype=dtype)
    n = P.shape[0]
    dP = DeviceBuffer(P)
    dX = DeviceBuffer(nbytes=n * n * P.itemsize, dtype=dtype, shape=(n, n))
    di = DeviceBuffer(nbytes=4, dtype=np.int32, shape=(1,))
    df = None
    if fixed is not None:
        fx = np.ascontiguousarray(np.asarray(fixed) != 0, dtype=np.uint8)
        if fx.shape != (n,):
            raise ValueError(f"fixed: {n} flags, not {fx.shape}")
        df = DeviceBuffer(fx)
    rc = getattr(L, "mir_lsq_spd_inverse_" + suf)(n, dP.ptr, df.ptr if df is not None else None, dX.ptr, di.ptr, None)
    if rc != 0:
        raise RuntimeError(f"mir_lsq_spd_inverse_{suf} failed: {rc}")
    X, info = dX.download(), int(di.download()[0])
    for b in (dP, dX, di, df):
        if b is not None:
            b.free()
    return X, info


def solveBoxQP(P, q, l, u, x=None, settings=None, dtype=np.float64, unconstrainedSolution=False):
    """argmin_x(1/2 xPx + qx) : l <= x <= u on the device (boxcqp.d:85-102 / 122-379).
    P: only the lower triangle is read. Returns (BoxQPStatus, x, active-set iterations)."""
    L = lib()
    P = np.ascontiguousarray(P, dtype=dtype)
    n = P.shape[0]
    q = np.ascontiguousarray(q, dtype=dtype)
    l = np.ascontiguousarray(l, dtype=dtype)
    u = np.ascontiguousarray(u, dtype=dtype)
    xo = np.zeros(n, dtype=dtype) if x is None else np.ascontiguousarray(x, dtype=dtype).copy()
    if settings is None:
        settings = BoxQPSettings(dtype)
    it = C.c_int(0)
    fn = L.mir_solve_box_qp_gpu_d if dtype == np.float64 else L.mir_solve_box_qp_gpu_s
    st = fn(C.byref(settings), n, P.ctypes.data, q.ctypes.data, l.ctypes.data, u.ctypes.data, xo.ctypes.data,
            1 if unconstrainedSolution else 0, C.byref(it))
    return BoxQPStatus(st), xo, it.value


BOX_QP_UNCONSTRAINED_SOLUTION = 1      # MIR_LSQ_BOX_QP_UNCONSTRAINED_SOLUTION

LM_SOLVE_KINDS = ("wave", "workgroup", "big")      # mir_lsq_lm_solve_class: out[0]
LM_SOLVE_SENTINEL = -123456.0                      # MIR_LSQ_LM_SOLVE_SENTINEL
LM_SOLVE_CHAIN = 8                                 # ladder entries of one launch, rows of dx / trial
LM_FLAG_DX_NAN, LM_FLAG_X_NAN, LM_FLAG_STEP_TOO_LONG, LM_FLAG_GRAD_SMALL, LM_FLAG_NULL_STEP, LM_FLAG_COOP_RESCUED = 1, 2, 4, 16, 32, 64


def lm_solve_class(elem_size, n, bounded, generic=False, diagnostic=False):
    """The kernel one LM solve launch runs (mir_lsq_lm_solve_class; host code, no GPU): (kind of LM_SOLVE_KINDS, LDS blocks a side
    the workgroup kernel is compiled for -- 0: factor in global memory --, True: the instance with the BOXCQP loop)."""
    out = (C.c_int * 3)()
    rc = lib().mir_lsq_lm_solve_class(elem_size, n, int(bool(bounded)), int(bool(generic)), int(bool(diagnostic)), C.byref(out))
    if rc != 0:
        raise ValueError(f"mir_lsq_lm_solve_class: {rc}")
    return LM_SOLVE_KINDS[out[0]], int(out[1]), bool(out[2])


def lm_solve_record_dtype(dtype):
    f = np.dtype(dtype)
    return np.dtype([("lambda", f), ("new_dx_dot", f), ("predicted", f), ("trial_xnorm", f), ("qp_status", np.int32),
                     ("qp_iterations", np.int32), ("flags", np.int32), ("reserved", np.int32)])


def lmSolve(JJ, Jy, x, lower, upper, lam, settings=None, dtype=np.float64, state_lambda=0.0, check_grad=False,
            lambda_from_state=False, force_bounded=False, generic=False, one_workgroup=False):
    """One launch of the LM solve kernels (mir_lsq_lm_solve_d / _s): the n x n part of a round for the ladder `lam` (1 .. 8 values).
    Returns a dict: rec (structured array, one record a ladder entry), dx, trial (8 x n; rows nobody wrote hold LM_SOLVE_SENTINEL),
    jy_inf, cls (as lm_solve_class), helpers (workgroups per ladder entry), guard (first damaged guard band or -1), bands, and
    inputs: (JJ, Jy, x, lower, upper) as they are on the device after the launch."""
    JJ = np.array(JJ, dtype=dtype, order="C")
    n = JJ.shape[0]
    if JJ.shape != (n, n):
        raise ValueError(f"JJ: n x n, not {JJ.shape}")
    vecs = [np.array(v, dtype=dtype, order="C") for v in (Jy, x, lower, upper)]
    if any(v.shape != (n,) for v in vecs):
        raise ValueError(f"Jy, x, lower, upper: {n} values each")
    lam = np.array(lam, dtype=dtype, order="C").reshape(-1)
    ks = lam.size
    if not 1 <= ks <= LM_SOLVE_CHAIN:
        raise ValueError(f"lam: 1 .. {LM_SOLVE_CHAIN} values, not {ks}")
    if settings is None:
        settings = LeastSquaresSettings(dtype)
    rec = np.zeros(ks, dtype=lm_solve_record_dtype(dtype))
    dx = np.zeros((LM_SOLVE_CHAIN, n), dtype=dtype)
    trial = np.zeros((LM_SOLVE_CHAIN, n), dtype=dtype)
    jy_inf = np.zeros(1, dtype=dtype)
    info = (C.c_int * 6)()
    mode = (1 if check_grad else 0) | (2 if lambda_from_state else 0) | (4 if force_bounded else 0) | (8 if generic else 0) \
        | (16 if one_workgroup else 0)
    fn = lib().mir_lsq_lm_solve_d if dtype == np.float64 else lib().mir_lsq_lm_solve_s
    rc = fn(C.byref(settings), n, JJ.ctypes.data, *(v.ctypes.data for v in vecs), ks, lam.ctypes.data, float(state_lambda), mode,
            rec.ctypes.data, dx.ctypes.data, trial.ctypes.data, jy_inf.ctypes.data, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_lm_solve failed: {rc}")
    return {"rec": rec, "dx": dx, "trial": trial, "jy_inf": jy_inf[0], "cls": (LM_SOLVE_KINDS[info[0]], int(info[1]), bool(info[2])),
            "helpers": int(info[3]), "guard": int(info[4]), "bands": int(info[5]), "inputs": (JJ, *vecs)}


LR_MAX = 16                 # kLrMax: pending rank-one terms of the read-only Broyden sweep (columns of U, rows of D)
LR_MAX_N = 512              # kLrMaxN
LR_MAX_BLOCKS = 1024        # kLrMaxBlocks


def lr_len(n):
    """length of a sweep's partial / reduced vector [ v0 (n) | g0 (n) | w (16) | h (16) | uu | uy | yy ]"""
    return 2 * n + 2 * LR_MAX + 3


def lr_class(elem_size, n, aligned=True):
    """The instance of the sweep and the flush kernels for n columns (mir_lsq_lr_class; host code, no GPU): (column-pair chunks a
    lane, True: vector loads)."""
    out = (C.c_int * 2)()
    rc = lib().mir_lsq_lr_class(elem_size, n, int(bool(aligned)), C.byref(out))
    if rc != 0:
        raise ValueError(f"mir_lsq_lr_class: {rc}")
    return int(out[0]), bool(out[1])


def lr_blocks(m, num_cu=0):
    """workgroups of the sweep for m rows (mir_lsq_lr_blocks); num_cu = 0: the current device's compute units (needs a GPU)"""
    rc = lib().mir_lsq_lr_blocks(m, num_cu)
    if rc < 1:
        raise ValueError(f"mir_lsq_lr_blocks: {rc}")
    return rc


def lrPass(m, n, k, J, U, D, dx, dx_dot, y, y_old, JJ, Jy, dtype=np.float64, count=1, spec=None, absTolerance=0.0, relTolerance=0.0,
           twh=None):
    """One Broyden pass of the read-only sweep on DEVICE pointers (mir_lsq_lr_pass_d / _s; the header has the contract). spec: None,
    or a dict with fields of lm_solve_record_dtype (the others zero). twh: a device pointer to n interval widths -- J is then the
    unscaled difference panel (mir_lsq_lr_pass_scaled_d; f64, n <= 256). Returns a dict: partials (nblk x lr_len(n)), reduced, sums
    (count), jy_inf, cls (as lr_class), nblk, guard (first damaged band of the call's own regions or -1), bands, touched."""
    dtype = np.dtype(dtype)
    if twh is not None and dtype != np.float64:
        raise ValueError("the scaled sweep exists in f64 only")
    nblk, ln = lr_blocks(m), lr_len(n)
    partials, reduced = np.zeros((nblk, ln), dtype=dtype), np.zeros(ln, dtype=dtype)
    sums, jy_inf = np.zeros(count, dtype=dtype), np.zeros(1, dtype=dtype)
    rec = None
    if spec is not None:
        rec = np.zeros(1, dtype=lm_solve_record_dtype(dtype))
        for key, v in spec.items():
            rec[key] = v
    info = (C.c_int * 6)()
    tail = (dx, dx_dot, y, count, y_old, JJ, Jy, rec.ctypes.data if rec is not None else None,
            float(absTolerance), float(relTolerance), partials.ctypes.data, reduced.ctypes.data, sums.ctypes.data, jy_inf.ctypes.data,
            C.byref(info))
    if twh is not None:
        rc = lib().mir_lsq_lr_pass_scaled_d(m, n, k, J, twh, U, D, *tail)
    else:
        fn = lib().mir_lsq_lr_pass_d if dtype == np.float64 else lib().mir_lsq_lr_pass_s
        rc = fn(m, n, k, J, U, D, *tail)
    if rc != 0:
        raise RuntimeError(f"mir_lsq_lr_pass failed: {rc}")
    if info[2] != nblk:
        raise RuntimeError(f"mir_lsq_lr_pass ran {info[2]} workgroups, mir_lsq_lr_blocks said {nblk}")
    return {"partials": partials, "reduced": reduced, "sums": sums, "jy_inf": jy_inf[0], "cls": (int(info[0]), bool(info[1])),
            "nblk": nblk, "guard": int(info[3]), "bands": int(info[4]), "touched": int(info[5])}


def lrFlush(m, n, k, J, U, D, dtype=np.float64):
    """J += the k pending terms, in place, on DEVICE pointers (mir_lsq_lr_flush_d / _s). Returns the class as lr_class."""
    info = (C.c_int * 2)()
    fn = lib().mir_lsq_lr_flush_d if np.dtype(dtype) == np.float64 else lib().mir_lsq_lr_flush_s
    rc = fn(m, n, k, J, U, D, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_lr_flush failed: {rc}")
    return int(info[0]), bool(info[1])


def lrFlushScaled(m, n, k, J, P, twh, U, D):
    """J = scale(P) + the k pending terms on DEVICE pointers (mir_lsq_lr_flush_scaled_d): P the unscaled difference panel, twh its
    widths; P is only read. Returns the class as lr_class (vector loads: even n, J and P both on the grid of two elements)."""
    info = (C.c_int * 2)()
    rc = lib().mir_lsq_lr_flush_scaled_d(m, n, k, J, P, twh, U, D, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_lr_flush_scaled failed: {rc}")
    return int(info[0]), bool(info[1])


LM_FLAG_TRIAL_NOT_FINITE = 8                     # kFlagTrialNotFinite (set by the decision, not by a solve)
LM_DECIDE_REJECT, LM_DECIDE_ACCEPT, LM_DECIDE_ACCEPT_NO_PREDICTION, LM_DECIDE_NUMERIC_ERROR, LM_DECIDE_GRAD_SMALL = 1, 2, 3, 4, 5
LM_STATE_FLOATS = ("lambda", "mu", "residual", "trial_residual", "dx_dot", "new_dx_dot", "predicted", "trial_xnorm", "jy_inf",
                   "improvement", "rho", "pad0")
LM_STATE_INTS = (("qp_status", np.int32), ("qp_iterations", np.int32), ("flags", np.int32), ("decision", np.int32),
                 ("iterations", np.uint32), ("accepted_k", np.int32), ("consumed", np.uint32), ("fcalls", np.uint32),
                 ("rejects", np.uint32), ("guards", np.uint32), ("qp_active", np.uint32), ("null_tail", np.uint32), ("seq", np.uint32),
                 ("coop_rescued", np.uint32), ("spec_ok", np.int32))


def lm_state_dtype(dtype):
    """mir_lsq_lm_state_d / _s (the kernels' LmState) as a structured dtype; in double the struct ends with 4 bytes of padding"""
    f = np.dtype(dtype)
    names = list(LM_STATE_FLOATS) + [k for k, _ in LM_STATE_INTS]
    formats = [f] * len(LM_STATE_FLOATS) + [t for _, t in LM_STATE_INTS]
    offsets = [i * f.itemsize for i in range(12)] + [12 * f.itemsize + 4 * i for i in range(len(LM_STATE_INTS))]
    size = 12 * f.itemsize + 4 * len(LM_STATE_INTS)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": -(-size // f.itemsize) * f.itemsize})


def lmDecide(state, rec, sums, x, trial, dx_chain, dx_acc, settings=None, dtype=np.float64, check_grad=False, lambda_from_state=False,
             spec_static=False, mirror=True, maxIterations=1000, seq=1, partials=None, nparts=0):
    """One launch of the decision kernel (mir_lsq_decide_d / _s; the header has the contract). state: one lm_state_dtype element,
    rec: ks lm_solve_record_dtype elements; partials: ks x pstride or None. Nothing passed in is written. Returns a dict of what
    is on the device after the launch -- state, rec, sums, x, trial, dx_chain, dx_acc, partials -- plus host_state, host_x (the
    pinned mirror; bytes of 0xFF without it), guard, bands."""
    dtype = np.dtype(dtype)
    state = np.array(state, dtype=lm_state_dtype(dtype)).reshape(1).copy()
    rec = np.array(rec, dtype=lm_solve_record_dtype(dtype)).reshape(-1).copy()
    ks = rec.size
    x, dx_acc = (np.array(v, dtype=dtype, order="C").reshape(-1) for v in (x, dx_acc))
    n = x.size
    sums = np.array(sums, dtype=dtype, order="C").reshape(-1)
    trial, dx_chain = (np.array(v, dtype=dtype, order="C") for v in (trial, dx_chain))
    if sums.shape != (ks,) or trial.shape != (ks, n) or dx_chain.shape != (ks, n) or dx_acc.shape != (n,):
        raise ValueError("lmDecide: sums ks, trial and dx_chain ks x n, x and dx_acc n values")
    pstride = 0
    if nparts:
        partials = np.array(partials, dtype=dtype, order="C")
        if partials.ndim != 2 or partials.shape[0] != ks:
            raise ValueError("lmDecide: partials ks x pstride")
        pstride = partials.shape[1]
    else:
        partials = None
    if settings is None:
        settings = LeastSquaresSettings(dtype.type)
    host_state = np.zeros(1, dtype=lm_state_dtype(dtype))
    host_x = np.zeros(n, dtype=dtype)
    info = (C.c_int * 2)()
    mode = (1 if check_grad else 0) | (2 if lambda_from_state else 0) | (4 if spec_static else 0) | (8 if mirror else 0)
    fn = lib().mir_lsq_decide_d if dtype == np.float64 else lib().mir_lsq_decide_s
    rc = fn(C.byref(settings), n, ks, mode, maxIterations, seq, state.ctypes.data, rec.ctypes.data, sums.ctypes.data, x.ctypes.data,
            trial.ctypes.data, dx_chain.ctypes.data, dx_acc.ctypes.data, partials.ctypes.data if partials is not None else None,
            nparts, pstride, host_state.ctypes.data, host_x.ctypes.data, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_decide failed: {rc}")
    return {"state": state, "rec": rec, "sums": sums, "x": x, "trial": trial, "dx_chain": dx_chain, "dx_acc": dx_acc,
            "partials": partials, "host_state": host_state, "host_x": host_x, "guard": int(info[0]), "bands": int(info[1])}


def fdPoints(x, lower, upper, eps, dtype=np.float64, with_base=False):
    """One launch of the finite-difference points (mir_lsq_fd_points_d / _s). Returns a dict: X ((2 n + with_base) x n), twh (the
    device's widths), twh_host (the solver's host copy of the same arithmetic), guard, bands."""
    dtype = np.dtype(dtype)
    x, lower, upper = (np.array(v, dtype=dtype, order="C").reshape(-1) for v in (x, lower, upper))
    n = x.size
    X = np.zeros((2 * n + (1 if with_base else 0), n), dtype=dtype)
    twh, twh_host = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    info = (C.c_int * 2)()
    fn = lib().mir_lsq_fd_points_d if dtype == np.float64 else lib().mir_lsq_fd_points_s
    rc = fn(n, x.ctypes.data, lower.ctypes.data, upper.ctypes.data, float(dtype.type(eps)), int(bool(with_base)), X.ctypes.data, twh.ctypes.data,
            twh_host.ctypes.data, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_fd_points failed: {rc}")
    return {"X": X, "twh": twh, "twh_host": twh_host, "guard": int(info[0]), "bands": int(info[1])}


def fdFill(Y, twh, J, j0, pc, dtype=np.float64, col=False):
    """One launch of the finite-difference column fill (mir_lsq_fd_fill_d / _s): Y 2 pc x ldy, twh n, J m x n (not written: the
    filled copy is returned), panel [j0, j0 + pc); col: the single-column kernel. Returns a dict: J, guard, bands."""
    dtype = np.dtype(dtype)
    Y, twh, J = np.array(Y, dtype=dtype, order="C"), np.array(twh, dtype=dtype, order="C").reshape(-1), np.array(J, dtype=dtype, order="C")
    m, n = J.shape
    if Y.shape[0] != 2 * pc or Y.shape[1] < m or twh.size != n:
        raise ValueError("fdFill: Y 2 pc x ldy with ldy >= m, twh n values")
    info = (C.c_int * 2)()
    fn = lib().mir_lsq_fd_fill_d if dtype == np.float64 else lib().mir_lsq_fd_fill_s
    rc = fn(m, n, Y.shape[1], j0, pc, Y.ctypes.data, twh.ctypes.data, J.ctypes.data, int(bool(col)), C.byref(info))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_fd_fill failed: {rc}")
    return {"J": J, "guard": int(info[0]), "bands": int(info[1])}


def sumsq_blocks(m):
    """workgroups of the entry residual's sum of squares (mir_lsq_sumsq_blocks; host code, no GPU)"""
    rc = lib().mir_lsq_sumsq_blocks(m)
    if rc < 1:
        raise ValueError(f"mir_lsq_sumsq_blocks: {rc}")
    return rc


def entryState(v, st2, dtype=np.float64, seq=1):
    """The entry of a solve (mir_lsq_entry_state_d / _s): v 2 x m (row 0 is the residual vector), st2 one lm_state_dtype element
    for the mu reset. Returns a dict: partials (nb), sum, state, host_state, partials2 (2 x nb), sums2 (2), st2, nb, guard, bands."""
    dtype = np.dtype(dtype)
    v = np.array(v, dtype=dtype, order="C")
    if v.ndim != 2 or v.shape[0] != 2:
        raise ValueError("entryState: v 2 x m")
    m = v.shape[1]
    nb = sumsq_blocks(m)
    partials, s, partials2, sums2 = np.zeros(nb, dtype=dtype), np.zeros(1, dtype=dtype), np.zeros((2, nb), dtype=dtype), np.zeros(2, dtype=dtype)
    state, host_state = np.zeros(1, dtype=lm_state_dtype(dtype)), np.zeros(1, dtype=lm_state_dtype(dtype))
    st2 = np.array(st2, dtype=lm_state_dtype(dtype)).reshape(1).copy()
    info = (C.c_int * 3)()
    fn = lib().mir_lsq_entry_state_d if dtype == np.float64 else lib().mir_lsq_entry_state_s
    rc = fn(m, v.ctypes.data, seq, partials.ctypes.data, s.ctypes.data, state.ctypes.data, host_state.ctypes.data, partials2.ctypes.data,
            sums2.ctypes.data, st2.ctypes.data, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_entry_state failed: {rc}")
    if info[0] != nb:
        raise RuntimeError(f"mir_lsq_entry_state ran {info[0]} workgroups, mir_lsq_sumsq_blocks said {nb}")
    return {"partials": partials, "sum": s[0], "state": state, "host_state": host_state, "partials2": partials2, "sums2": sums2,
            "st2": st2, "nb": nb, "guard": int(info[1]), "bands": int(info[2])}


def unpackGrad(packed, n, state, dtype=np.float64):
    """One launch that expands the packed [J^T J lower | J^T y] buffer (mir_lsq_unpack_grad_d / _s). Returns a dict: JJ, Jy, state
    (the image after the launch: jy_inf written), guard, bands."""
    dtype = np.dtype(dtype)
    packed = np.array(packed, dtype=dtype, order="C").reshape(-1)
    if packed.size != n * (n + 1) // 2 + n:
        raise ValueError("unpackGrad: n (n + 1) / 2 + n values")
    state = np.array(state, dtype=lm_state_dtype(dtype)).reshape(1).copy()
    JJ, Jy = np.zeros((n, n), dtype=dtype), np.zeros(n, dtype=dtype)
    info = (C.c_int * 2)()
    fn = lib().mir_lsq_unpack_grad_d if dtype == np.float64 else lib().mir_lsq_unpack_grad_s
    rc = fn(n, packed.ctypes.data, state.ctypes.data, JJ.ctypes.data, Jy.ctypes.data, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_unpack_grad failed: {rc}")
    return {"JJ": JJ, "Jy": Jy, "state": state, "guard": int(info[0]), "bands": int(info[1])}


def _box_qp_batched_pack(P, q, l, u, x, dtype, unconstrainedSolution):
    """The 8-wide layout of mir_lsq_batched_box_qp_* from count x n x n / count x n arrays (host side, no device): returns
    (count, n, P count x 8 x 8, q count x 8, l, u (8,) or count x 8, bound_stride, x count x 8). Raises ValueError."""
    return _box_qp_batched_pack_w(P, q, l, u, x, dtype, unconstrainedSolution, 8, 1)


def _box_qp_batched_pack16(P, q, l, u, x, dtype, unconstrainedSolution):
    """The 16-wide layout of mir_lsq_batched_box_qp16_* (n = 9 .. 16), by the rules of _box_qp_batched_pack: returns
    (count, n, P count x 16 x 16, q count x 16, l, u (16,) or count x 16, bound_stride 0 or 16, x count x 16)."""
    return _box_qp_batched_pack_w(P, q, l, u, x, dtype, unconstrainedSolution, 16, 9)


def _box_qp_batched_pack_w(P, q, l, u, x, dtype, unconstrainedSolution, W, nmin):
    """what the two layouts share: validation and zero padding to W-wide rows for nmin <= n <= W"""
    suf = _batched_suffix(dtype)
    dtype = np.float32 if suf == "s" else np.float64
    P = np.asarray(P, dtype=dtype)
    if P.ndim != 3 or P.shape[1] != P.shape[2]:
        raise ValueError(f"P: count x n x n, not {P.shape}")
    count, n = P.shape[0], P.shape[1]
    if not nmin <= n <= W:
        raise ValueError(f"solveBoxQPBatched: n = {n} is outside {nmin} .. {W}")
    q = np.asarray(q, dtype=dtype)
    if q.shape != (count, n):
        raise ValueError(f"q: {count} x {n}, not {q.shape}")
    l, u = np.asarray(l, dtype=dtype), np.asarray(u, dtype=dtype)
    if l.shape != u.shape or l.shape not in ((n,), (count, n)):
        raise ValueError(f"l, u: both {n} values or both {count} x {n}, not {l.shape} and {u.shape}")
    shared = l.ndim == 1
    Pp = np.zeros((count, W, W), dtype=dtype); Pp[:, :n, :n] = P
    qp = np.zeros((count, W), dtype=dtype); qp[:, :n] = q
    lp = np.zeros((W,) if shared else (count, W), dtype=dtype); lp[..., :n] = l
    up = np.zeros((W,) if shared else (count, W), dtype=dtype); up[..., :n] = u
    xp = np.zeros((count, W), dtype=dtype)
    if x is not None:
        x = np.asarray(x, dtype=dtype)
        if x.shape != (count, n):
            raise ValueError(f"x: {count} x {n}, not {x.shape}")
        xp[:, :n] = x
    elif unconstrainedSolution:
        raise ValueError("unconstrainedSolution=True needs x, the unconstrained minimisers")
    return count, n, Pp, qp, lp, up, (0 if shared else W), xp


def solveBoxQPBatched(P, q, l, u, x=None, settings=None, dtype=np.float64, unconstrainedSolution=False):
    """`count` solveBoxQP problems of order n <= 16 in one launch, four problems a wavefront (n <= 8: mir_lsq_batched_box_qp_d
    / _s in the 8-wide layout; n = 9 .. 16: mir_lsq_batched_box_qp16_d / _s in the 16-wide one):
    argmin_x(1/2 xPx + qx) : l <= x <= u for every problem. P count x n x n (lower triangles read), q count x n, l and u
    n values shared by all problems or count x n; x (only with unconstrainedSolution=True): the unconstrained minimisers,
    count x n. Returns (status[count] of BoxQPStatus values, x[count, n], iterations[count])."""
    n_in = np.shape(P)[1] if np.ndim(P) == 3 else 0
    if n_in > 16:
        raise ValueError(f"solveBoxQPBatched: n = {n_in} is above 16, the limit of the batched kernels")
    wide = n_in > 8
    pack = _box_qp_batched_pack16 if wide else _box_qp_batched_pack
    count, n, Pp, qp, lp, up, bound_stride, xp = pack(P, q, l, u, x, dtype, unconstrainedSolution)
    dtype = Pp.dtype.type
    suf = "s" if dtype == np.float32 else "d"
    if settings is None:
        settings = BoxQPSettings(dtype)
    if count == 0:
        return np.zeros(0, dtype=np.int32), np.zeros((0, n), dtype=dtype), np.zeros(0, dtype=np.int32)
    L = lib()
    bufs = [DeviceBuffer(a) for a in (Pp, qp, lp, up, xp)]
    dst = DeviceBuffer(nbytes=count * 4, dtype=np.int32, shape=(count,))
    dit = DeviceBuffer(nbytes=count * 4, dtype=np.int32, shape=(count,))
    st = Stream()
    name = ("mir_lsq_batched_box_qp16_" if wide else "mir_lsq_batched_box_qp_") + suf
    rc = getattr(L, name)(C.addressof(settings), count, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bound_stride,
                          bufs[4].ptr, dst.ptr, dit.ptr, BOX_QP_UNCONSTRAINED_SOLUTION if unconstrainedSolution else 0, st.handle)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {rc}")
    st.synchronize()
    out = dst.download().copy(), bufs[4].download()[:, :n].copy(), dit.download().copy()
    for b in bufs + [dst, dit]:
        b.free()
    return out


BOX_QP_WIDE_ORDERS = (17, 64)         # mir_lsq_batched_box_qp64_*: the orders it takes


def _box_qp_batched_pack_dense(P, q, l, u, x, dtype, unconstrainedSolution):
    """The dense layout of mir_lsq_batched_box_qp64_* (n = 17 .. 64) from count x n x n / count x n arrays (host side, no
    device), by the rules of _box_qp_batched_pack_w without the padding: returns (count, n, P count x n x n, q count x n, l, u
    (n,) or count x n, bound_stride 0 or n, x count x n), C-contiguous arrays of `dtype`. Raises ValueError."""
    suf = _batched_suffix(dtype)
    dtype = np.float32 if suf == "s" else np.float64
    P = np.ascontiguousarray(P, dtype=dtype)
    if P.ndim != 3 or P.shape[1] != P.shape[2]:
        raise ValueError(f"P: count x n x n, not {P.shape}")
    count, n = P.shape[0], P.shape[1]
    nmin, nmax = BOX_QP_WIDE_ORDERS
    if not nmin <= n <= nmax:
        raise ValueError(f"solveBoxQPBatchedWide: n = {n} is outside {nmin} .. {nmax}")
    q = np.ascontiguousarray(q, dtype=dtype)
    if q.shape != (count, n):
        raise ValueError(f"q: {count} x {n}, not {q.shape}")
    l, u = np.ascontiguousarray(l, dtype=dtype), np.ascontiguousarray(u, dtype=dtype)
    if l.shape != u.shape or l.shape not in ((n,), (count, n)):
        raise ValueError(f"l, u: both {n} values or both {count} x {n}, not {l.shape} and {u.shape}")
    if x is not None:
        xp = np.array(x, dtype=dtype, order="C")
        if xp.shape != (count, n):
            raise ValueError(f"x: {count} x {n}, not {xp.shape}")
    elif unconstrainedSolution:
        raise ValueError("unconstrainedSolution=True needs x, the unconstrained minimisers")
    else:
        xp = np.zeros((count, n), dtype=dtype)
    return count, n, P, q, l, u, (0 if l.ndim == 1 else n), xp


def solveBoxQPBatchedWide(P, q, l, u, x=None, settings=None, dtype=np.float64, unconstrainedSolution=False, max_waves=0):
    """`count` solveBoxQP problems of order n = 17 .. 64 in one launch (mir_lsq_batched_box_qp64_d / _s: one problem a wavefront
    at n > 32, two at n <= 32, the matrices in LDS): argmin_x(1/2 xPx + qx) : l <= x <= u for every problem. Arguments and
    results as solveBoxQPBatched's: P count x n x n (lower triangles read), q count x n, l and u n values shared by all problems
    or count x n; x (only with unconstrainedSolution=True): the unconstrained minimisers. max_waves: a cap on the wavefronts
    launched (mir_lsq_batched_box_qp64_waves_*; 0: the default) -- the answers do not depend on it. Returns (status[count] of
    BoxQPStatus values, x[count, n], iterations[count]). Raises ValueError for an order outside 17 .. 64."""
    count, n, Pp, qp, lp, up, bound_stride, xp = _box_qp_batched_pack_dense(P, q, l, u, x, dtype, unconstrainedSolution)
    dtype = Pp.dtype.type
    suf = "s" if dtype == np.float32 else "d"
    if settings is None:
        settings = BoxQPSettings(dtype)
    if count == 0:
        return np.zeros(0, dtype=np.int32), np.zeros((0, n), dtype=dtype), np.zeros(0, dtype=np.int32)
    L = lib()
    bufs = [DeviceBuffer(a) for a in (Pp, qp, lp, up, xp)]
    dst = DeviceBuffer(nbytes=count * 4, dtype=np.int32, shape=(count,))
    dit = DeviceBuffer(nbytes=count * 4, dtype=np.int32, shape=(count,))
    st = Stream()
    name = "mir_lsq_batched_box_qp64_waves_" + suf
    rc = getattr(L, name)(C.addressof(settings), count, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bound_stride,
                          bufs[4].ptr, dst.ptr, dit.ptr, BOX_QP_UNCONSTRAINED_SOLUTION if unconstrainedSolution else 0, st.handle,
                          int(max_waves))
    if rc != 0:
        raise RuntimeError(f"{name} failed: {rc}")
    st.synchronize()
    out = dst.download().copy(), bufs[4].download().copy(), dit.download().copy()
    for b in bufs + [dst, dit]:
        b.free()
    return out


def jtj(J, y, y_old=None, dx=None, dtype=np.float64):
    """Unit-level access to the J^T J + J^T y kernels (mir_lsq_jtj_*; with dx: the Broyden REWRITE kernels, the literal
    restatement of LS:1003-1006). Returns (JJ full symmetric, Jy, J_after, kernel_ms).
    J is uploaded to the start of an allocation, so it is always 16-byte aligned here. The C entries also take a J that is an
    element-aligned view (jtj_resolve in csrc/jtj_plan.h reroutes the kernels that need 16-byte loads); y, y_old and dx must stay
    16-byte aligned. tests/jtj_cases.run_jtj drives the entries that way, between NaN guard bands, for every instantiated kernel
    class -- except the eight-wave ring (f64, 128 < n <= 256, n % 16 == 0, even m) at an offset J, which is not established to be
    defined and is not run (see the header comment of jtj_plan.h)."""
    L = lib()
    J = np.ascontiguousarray(J, dtype=dtype)
    m, n = J.shape
    dJ = DeviceBuffer(J)
    dy = DeviceBuffer(np.ascontiguousarray(y, dtype=dtype))
    broyden = dx is not None
    dyo = DeviceBuffer(np.ascontiguousarray(y_old if broyden else y, dtype=dtype))
    ddx = DeviceBuffer(np.ascontiguousarray(dx if broyden else np.zeros(n), dtype=dtype))
    dJJ = DeviceBuffer(nbytes=n * n * J.itemsize, dtype=dtype, shape=(n, n))
    dJy = DeviceBuffer(nbytes=n * J.itemsize, dtype=dtype, shape=(n,))
    ms = C.c_float(0)
    fn = L.mir_lsq_jtj_d if dtype == np.float64 else L.mir_lsq_jtj_s
    rc = fn(m, n, dJ.ptr, dy.ptr, dyo.ptr, ddx.ptr, 1 if broyden else 0, dJJ.ptr, dJy.ptr, None, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_jtj failed: {rc}")
    out = dJJ.download(), dJy.download(), dJ.download(), ms.value
    for b in (dJ, dy, dyo, ddx, dJJ, dJy):
        b.free()
    return out


JTJ_OPS = ("plain", "rewrite", "fd", "fd_diff", "fd_diff_keep")
JTJ_FAMILIES = ("none", "stream", "fdp", "pc32", "ring8", "fdp8", "wide", "fdp_nw")


def jtj_plan(elem_size, m, n, num_cu, op, aligned=True):
    """The kernel the J^T J entries launch for a shape and an operation of JTJ_OPS (mir_lsq_jtj_plan; host code, no GPU).
    Returns a dict: family (of JTJ_FAMILIES), ncb, flat, grid, jobs, lds, slabs, slab_len, reduce_ncb, workspace_slab_elems."""
    out = (C.c_size_t * 10)()
    rc = lib().mir_lsq_jtj_plan(elem_size, m, n, num_cu, JTJ_OPS.index(op), int(bool(aligned)), C.byref(out))
    if rc != 0:
        raise ValueError(f"mir_lsq_jtj_plan: {rc}")
    d = dict(zip(("family", "ncb", "flat", "grid", "jobs", "lds", "slabs", "slab_len", "reduce_ncb", "workspace_slab_elems"), map(int, out)))
    d["family"] = JTJ_FAMILIES[d["family"]]
    return d


def fd_jtj(Yrm, twh, y, diff=False, write_J=True):
    """Unit-level access to the J^T J kernel with the finite-difference fill fused in (mir_lsq_fd_jtj_d).
    Yrm: m x 2n row-major (+h / -h residual pairs) -- or, diff=True, the m x n difference panel (mir_lsq_fd_diff_jtj_d).
    write_J=False (diff only): a NULL J, as the solver's default refresh passes it; the J returned is None.
    Returns (J, JJ full symmetric, Jy, kernel_ms)."""
    if not write_J and not diff:
        raise ValueError("only the difference-panel kernel takes a NULL J")
    L = lib()
    Yrm = np.ascontiguousarray(Yrm, dtype=np.float64)
    m, n2 = Yrm.shape
    n = n2 if diff else n2 // 2
    dY = DeviceBuffer(Yrm)
    dt = DeviceBuffer(np.ascontiguousarray(twh, dtype=np.float64))
    dy = DeviceBuffer(np.ascontiguousarray(y, dtype=np.float64))
    dJ = DeviceBuffer(nbytes=m * n * 8, dtype=np.float64, shape=(m, n))
    dJJ = DeviceBuffer(nbytes=n * n * 8, dtype=np.float64, shape=(n, n))
    dJy = DeviceBuffer(nbytes=n * 8, dtype=np.float64, shape=(n,))
    ms = C.c_float(0)
    rc = (L.mir_lsq_fd_diff_jtj_d if diff else L.mir_lsq_fd_jtj_d)(m, n, dY.ptr, dt.ptr, dy.ptr, dJ.ptr if write_J else None, dJJ.ptr, dJy.ptr, None, C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"mir_lsq_fd_jtj_d failed: {rc}")
    out = dJ.download() if write_J else None, dJJ.download(), dJy.download(), ms.value
    for b in (dY, dt, dy, dJ, dJJ, dJy):
        b.free()
    return out


# ---- fitSpline (fit_splie.d:26-85): a caller of the LM path -----------------------------------------------

class Spline:
    """C2 cubic spline with not-a-knot ends in Hermite form (what mir.interpolate.spline's default configuration
    builds); evaluation and derivatives go through the library's host code (mir_spline_*)."""

    def __init__(self, x, values, dtype=np.float64):
        self.dtype = dtype
        self.x = np.ascontiguousarray(x, dtype=dtype)
        self.values = np.ascontiguousarray(values, dtype=dtype)
        self.derivatives = np.zeros_like(self.values)
        suf = "d" if dtype == np.float64 else "s"
        getattr(lib(), "mir_spline_c2_derivatives_" + suf)(self.x.size, self.x.ctypes.data, self.values.ctypes.data,
                                                         self.derivatives.ctypes.data)
        self._eval = getattr(lib(), "mir_spline_eval_" + suf)

    def withTwoDerivatives(self, t):
        out = np.zeros(3, dtype=self.dtype)
        self._eval(self.x.size, self.x.ctypes.data, self.values.ctypes.data, self.derivatives.ctypes.data, t, out.ctypes.data)
        return out

    def __call__(self, t):
        if np.ndim(t) == 0:
            return self.withTwoDerivatives(float(t))[0]
        return np.array([self.withTwoDerivatives(float(v))[0] for v in np.asarray(t).ravel()]).reshape(np.shape(t))


class FitSplineResult:
    """FitSplineResult!T (fit_splie.d:7-13)."""

    def __init__(self, leastSquaresResult, spline):
        self.leastSquaresResult = leastSquaresResult
        self.spline = spline


def fit_spline_residuals(points, x, lambda_, splineY):
    """The residual vector fitSpline minimises (FS:60-84), from the library's host code (double)."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    v = np.ascontiguousarray(splineY, dtype=np.float64)
    m = points.shape[0] + (1 if lambda_ == 0 else 0)
    y = np.zeros(m)
    lib().mir_fit_spline_residuals_d(points.shape[0], points.ctypes.data, x.size, x.ctypes.data, lambda_, v.ctypes.data, m,
                                     y.ctypes.data)
    return y


def fitSpline(settings, points, x, l, u, lambda_=0.0, dtype=np.float64):
    """fitSpline (fit_splie.d:26-85): least-squares fit of the spline values at the fixed knots `x` to `points`
    (k x 2), bounds l <= spline(x) <= u, optional smoothness weight lambda_. Raises like the reference: Exception for
    too few points (FS:47-51), LeastSquaresException for a negative LM status (through `optimize`, LS:175-179)."""
    L = lib()
    points = np.ascontiguousarray(points, dtype=dtype)
    x = np.ascontiguousarray(x, dtype=dtype)
    lo = np.ascontiguousarray(l, dtype=dtype)
    up = np.ascontiguousarray(u, dtype=dtype)
    if not lambda_ >= 0:
        raise ValueError("fitSpline: lambda has to be non-negative")        # the reference's in-contract
    y = np.zeros(x.size, dtype=dtype)
    d = np.zeros(x.size, dtype=dtype)
    dbl = dtype == np.float64
    raw = (_Rd if dbl else _Rs)()
    fn = L.mir_fit_spline_d if dbl else L.mir_fit_spline_s
    rc = fn(C.byref(settings) if settings is not None else None, points.shape[0], points.ctypes.data, x.size,
            x.ctypes.data, lo.ctypes.data, up.ctypes.data, lambda_, None, y.ctypes.data, d.ctypes.data, C.byref(raw))
    if rc == 1:
        raise Exception("fitSpline: points.length has to be greater or equal x.length when lambda is 0.0")
    if rc != 0:
        raise ValueError("fitSpline: bad argument")
    res = LeastSquaresResult(raw)
    if res.status < 0:
        raise LeastSquaresException(int(res.status), res)
    return FitSplineResult(res, Spline(x, y, dtype))


# ---- fitSpline on device-resident points (csrc/fit_spline_gpu.hip): the residuals as kernels -------------------------

def fitSplineGpu(settings, points, x, l, u, lambda_=0.0, dtype=np.float64, stats=None, variant=0, stream=None):
    """fitSpline through the GPU-native contract (mir_fit_spline_gpu_*): `points` is a numpy array (k x 2, uploaded) or a
    DeviceBuffer of that shape and dtype; everything else, the result and the exceptions are those of fitSpline. stats: an
    optional Stats to fill (kernels are event-timed then), variant: MIR_LSQ_VARIANT_* bits, stream: an optional Stream."""
    L = lib()
    x = np.ascontiguousarray(x, dtype=dtype)
    lo = np.ascontiguousarray(l, dtype=dtype)
    up = np.ascontiguousarray(u, dtype=dtype)
    if not lambda_ >= 0:
        raise ValueError("fitSpline: lambda has to be non-negative")
    own = not isinstance(points, DeviceBuffer)
    if own:
        points = np.ascontiguousarray(points, dtype=dtype)
        if points.ndim != 2 or points.shape[1] != 2:
            raise ValueError("fitSplineGpu: points has to be k x 2")
        k = points.shape[0]
        if k < x.size and lambda_ == 0:
            raise Exception("fitSpline: points.length has to be greater or equal x.length when lambda is 0.0")
        if k == 0:
            raise ValueError("fitSpline: bad argument")
        dev = DeviceBuffer(points)
    else:
        dev = points
        if len(dev.shape) != 2 or dev.shape[1] != 2 or dev.dtype != np.dtype(dtype):
            raise ValueError("fitSplineGpu: points has to be a k x 2 DeviceBuffer of the fit's dtype")
        k = dev.shape[0]
    opt = GpuOptions(variant=variant)
    if stats is not None:
        opt.stats = C.pointer(stats)
        opt.flags = TIME_KERNELS
    if stream is not None:
        opt.stream = stream.handle
    y = np.zeros(x.size, dtype=dtype)
    d = np.zeros(x.size, dtype=dtype)
    dbl = dtype == np.float64
    raw = (_Rd if dbl else _Rs)()
    fn = L.mir_fit_spline_gpu_d if dbl else L.mir_fit_spline_gpu_s
    try:
        rc = fn(C.byref(settings) if settings is not None else None, k, dev.ptr, x.size, x.ctypes.data, lo.ctypes.data,
                up.ctypes.data, lambda_, C.byref(opt), y.ctypes.data, d.ctypes.data, C.byref(raw))
    finally:
        if own:
            dev.free()
    if rc == 1:
        raise Exception("fitSpline: points.length has to be greater or equal x.length when lambda is 0.0")
    if rc != 0:
        raise ValueError("fitSpline: bad argument")
    res = LeastSquaresResult(raw)
    if res.status < 0:
        raise LeastSquaresException(int(res.status), res)
    return FitSplineResult(res, Spline(x, y, dtype))


def splineEvalGpu(spline, t, stream=None):
    """Values of a Spline at many abscissae on the device (mir_spline_eval_gpu_*): t is a numpy array (uploaded; a numpy array
    of its shape comes back) or a 1-D DeviceBuffer of the spline's dtype (a DeviceBuffer comes back)."""
    dtype = spline.dtype
    suf = "d" if dtype == np.float64 else "s"
    own = not isinstance(t, DeviceBuffer)
    if own:
        ta = np.ascontiguousarray(t, dtype=dtype)
        shape = ta.shape
        if ta.size == 0:
            return np.zeros(shape, dtype=dtype)
        dt = DeviceBuffer(ta.ravel())
    else:
        dt = t
        if dt.dtype != np.dtype(dtype):
            raise ValueError("splineEvalGpu: t has to have the spline's dtype")
    count = int(np.prod(dt.shape))
    out = DeviceBuffer(nbytes=count * np.dtype(dtype).itemsize, dtype=dtype, shape=(count,))
    rc = getattr(lib(), "mir_spline_eval_gpu_" + suf)(spline.x.size, spline.x.ctypes.data, spline.values.ctypes.data,
                                                       spline.derivatives.ctypes.data, count, dt.ptr, out.ptr,
                                                       stream.handle if stream is not None else None)
    if rc != 0:
        raise RuntimeError(f"mir_spline_eval_gpu_{suf} failed: {rc}")
    if not own:
        return out
    v = out.download().reshape(shape)
    out.free()
    dt.free()
    return v


def _fit_spline_eval(name, points_ptr, npoints, x, lambda_, X, mode, dtype):
    x = np.ascontiguousarray(x, dtype=dtype)
    X = np.ascontiguousarray(X, dtype=dtype).reshape(-1, x.size)
    p, nx = X.shape
    m = npoints + (1 if lambda_ == 0 else 0)
    out = np.zeros(p * m if mode == 0 else m * nx + (m if p == 2 * nx + 1 else 0), dtype=dtype)
    suf = "d" if dtype == np.float64 else "s"
    rc = getattr(lib(), name + suf)(npoints, points_ptr, nx, x.ctypes.data, lambda_, p, X.ctypes.data, mode, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"{name}{suf} failed: {rc}")
    return out.reshape(p, m) if mode == 0 else out


def fit_spline_eval_host(points, x, lambda_, X, mode=0, dtype=np.float64):
    """mir_fit_spline_eval_host_*: the residual callbacks of fitSplineGpu on the CPU (the shared arithmetic of
    csrc/spline_c2.h). X: p value vectors. mode 0: the p x m residual vectors; mode 1 (p = 2 nx or 2 nx + 1): the flat
    m x nx difference panel, followed by the m residuals of the last vector when p = 2 nx + 1."""
    points = np.ascontiguousarray(points, dtype=dtype)
    return _fit_spline_eval("mir_fit_spline_eval_host_", points.ctypes.data, points.shape[0], x, lambda_, X, mode, dtype)


def fit_spline_eval_gpu(points, x, lambda_, X, mode=0, dtype=np.float64):
    """mir_fit_spline_gpu_eval_*: the per-fit setup of fitSplineGpu and then exactly the callback a solve would call (mode 0:
    fb, mode 1: fbRowMajorDiff, double). points: numpy (uploaded) or a k x 2 DeviceBuffer. Results as fit_spline_eval_host."""
    own = not isinstance(points, DeviceBuffer)
    dev = DeviceBuffer(np.ascontiguousarray(points, dtype=dtype)) if own else points
    try:
        return _fit_spline_eval("mir_fit_spline_gpu_eval_", dev.ptr, dev.shape[0], x, lambda_, X, mode, dtype)
    finally:
        if own:
            dev.free()


def fit_spline_factor(x, dtype=np.float64):
    """mir_fit_spline_factor_*: the factor of the knots' not-a-knot system as a dict of its five arrays (di, up, up2, f after
    the elimination; swap[i] = 1 where step i exchanged rows)."""
    x = np.ascontiguousarray(x, dtype=dtype)
    F = np.zeros(5 * x.size, dtype=dtype)
    rc = getattr(lib(), "mir_fit_spline_factor_" + ("d" if dtype == np.float64 else "s"))(x.size, x.ctypes.data, F.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"mir_fit_spline_factor failed: {rc}")
    return dict(zip(("di", "up", "up2", "f", "swap"), F.reshape(5, x.size)))
