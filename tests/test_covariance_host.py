"""Host side of the covariance step and of the SPD inverse (include/mir_optim_amd.h: mir_lsq_covariance_gpu_*,
mir_lsq_spd_inverse_*): the symbols, the ctypes mirror and the argument checks that are answered before a device is touched.
No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np

import mir_optim_amd as M
from mir_optim_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mir_lsq_covariance_gpu_d", "mir_lsq_covariance_gpu_s", "mir_lsq_spd_inverse_d", "mir_lsq_spd_inverse_s")


def test_symbols_are_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = api.lib()
    for nm in NAMES + ("mir_lsq_spd_inverse_work_d", "mir_lsq_spd_inverse_work_s", "mir_lsq_spd_inverse_work_bytes"):
        assert re.search(r"\b" + nm + r"\s*\(", src), nm
        assert hasattr(L, nm), nm
    assert re.search(r"MIR_LSQ_COVARIANCE_ABSOLUTE_SIGMA\s*=\s*1u", src)
    assert M.COVARIANCE_ABSOLUTE_SIGMA == 1
    assert api.lib().mir_lsq_version().startswith(b"mir_optim_amd 0.4")
    assert C.sizeof(api.GpuOptions) == 96


def test_ctypes_mirror_matches_the_prototypes():
    L = api.lib()
    for suf, S in (("d", api._Sd), ("s", api._Ss)):
        fn = getattr(L, "mir_lsq_covariance_gpu_" + suf)
        assert fn.restype is C.c_int and len(fn.argtypes) == 17
        assert fn.argtypes[0] is C.POINTER(S) and fn.argtypes[6] is C.POINTER(api.GpuOptions)
        assert fn.argtypes[13] is C.c_uint32 and fn.argtypes[16] is C.POINTER(C.c_int)
        fn = getattr(L, "mir_lsq_spd_inverse_" + suf)
        assert fn.restype is C.c_int and len(fn.argtypes) == 6
        assert len(getattr(L, "mir_lsq_spd_inverse_work_" + suf).argtypes) == 8
    assert L.mir_lsq_spd_inverse_work_bytes(10, 8) == (100 + 10) * 8 and L.mir_lsq_spd_inverse_work_bytes(10, 4) == 440
    assert L.mir_lsq_spd_inverse_work_bytes(10, 2) == 0


def _raw(dtype, x, l, u, cov=True, f=True, settings=None, m=4, n=None):
    """mir_lsq_covariance_gpu_* with raw pointers; f is never called by the paths tested here"""
    ct = C.c_double if dtype == np.float64 else C.c_float
    ft = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(ct), C.POINTER(ct))
    called = []
    thunk = ft(lambda *a: called.append(1))
    s = settings if settings is not None else M.LeastSquaresSettings(dtype)
    arr = [None if v is None else np.ascontiguousarray(v, dtype=dtype) for v in (x, l, u)]
    nn = n if n is not None else (arr[0].size if arr[0] is not None else 2)
    out = np.full((max(nn, 1), max(nn, 1)), 7.0, dtype=dtype)
    info = C.c_int(-5)
    fn = getattr(api.lib(), "mir_lsq_covariance_gpu_" + ("d" if dtype == np.float64 else "s"))
    rc = fn(C.byref(s), m, nn, *[None if a is None else a.ctypes.data for a in arr], None, None,
            C.cast(thunk, C.c_void_p) if f else None, None, None, None, None, 0, out.ctypes.data if cov else None, None, C.byref(info))
    assert not called and np.all(out == 7.0) and info.value == -5       # nothing evaluated, nothing written
    return rc


def test_argument_checks_answer_without_a_device():
    lo, up = [-1.0, -1.0], [1.0, 1.0]
    for dt in (np.float64, np.float32):
        assert _raw(dt, None, lo, up) == -31                             # x NULL
        assert _raw(dt, [0.0, 0.0], lo, up, n=0) == -31                  # n == 0
        assert _raw(dt, [0.0, 0.0], lo, up, m=0) == -31                  # m == 0
        assert _raw(dt, [np.nan, 0.0], lo, up) == -31 and _raw(dt, [0.0, np.inf], lo, up) == -31
        assert _raw(dt, [0.0, 0.0], lo, up, cov=False) == -1             # cov NULL
        assert _raw(dt, [0.0, 0.0], lo, up, f=False) == -1               # f NULL
        assert _raw(dt, [0.0, 0.0], None, up) == -1 and _raw(dt, [0.0, 0.0], lo, None) == -1
        assert _raw(dt, [2.0, 0.0], lo, up) == -32 and _raw(dt, [0.0, -1.5], lo, up) == -32
        for field, val, code in (("minStepQuality", 1.0, -30), ("goodStepQuality", 1.5, -29), ("goodStepQuality", 0.05, -28),
                                 ("lambdaIncrease", 0.5, -27)):
            s = M.LeastSquaresSettings(dt)
            setattr(s, field, val)
            assert _raw(dt, [0.0, 0.0], lo, up, settings=s) == code, field
    # the validation order of the solve: the guess before the bounds before the settings
    s = M.LeastSquaresSettings(); s.minStepQuality = 1.0
    assert _raw(np.float64, [np.nan, 5.0], lo, up, settings=s) == -31 and _raw(np.float64, [0.0, 5.0], lo, up, settings=s) == -32


def _raw_solve(dtype, x, l, u, settings=None, m=4):
    """mir_optimize_least_squares_gpu_* with raw pointers; f is never called by the paths tested here"""
    ct = C.c_double if dtype == np.float64 else C.c_float
    ft = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(ct), C.POINTER(ct))
    called = []
    thunk = ft(lambda *a: called.append(1))
    s = settings if settings is not None else M.LeastSquaresSettings(dtype)
    xa, la, ua = (np.ascontiguousarray(v, dtype=dtype) for v in (x, l, u))
    x0 = xa.copy()
    fn = getattr(api.lib(), "mir_optimize_least_squares_gpu_" + ("d" if dtype == np.float64 else "s"))
    r = fn(C.byref(s), m, xa.size, xa.ctypes.data, la.ctypes.data, ua.ctypes.data, None, None, C.cast(thunk, C.c_void_p),
           None, None, None, None)
    assert not called and r.iterations == 0 and r.fCalls == 0 and r.gCalls == 0    # nothing evaluated
    assert np.array_equal(xa, x0, equal_nan=True)                                 # x untouched
    return r.status


def test_the_solve_and_the_covariance_step_share_one_validation():
    """LS:930-943 is one function for both entry points: the same status for every invalid input, in the same order (the guess
    before the bounds before the settings), answered before a device is asked for and before f is called."""
    lo, up = [-1.0, -1.0], [1.0, 1.0]
    good = [0.0, 0.0]
    bad_set = (("minStepQuality", 1.0, -30), ("minStepQuality", -0.5, -30), ("goodStepQuality", 1.5, -29),
               ("goodStepQuality", 0.05, -28), ("lambdaIncrease", 0.5, -27), ("lambdaDecrease", 2.0, -27))
    for dt in (np.float64, np.float32):
        def worst():
            s = M.LeastSquaresSettings(dt)
            s.minStepQuality = 1.0
            return s
        rows = [(x, lo, up, None, 4, -31) for x in ([np.nan, 0.0], [0.0, np.nan], [np.inf, 0.0], [0.0, -np.inf])]
        rows += [(good, lo, up, None, 0, -31)]                           # m == 0
        rows += [([-1.5, 0.0], lo, up, None, 4, -32), ([0.0, -2.0], lo, up, None, 4, -32)]     # x below l
        rows += [([2.0, 0.0], lo, up, None, 4, -32), ([0.0, 1.5], lo, up, None, 4, -32)]       # x above u
        rows += [(good, [np.nan, -1.0], up, None, 4, -32), (good, lo, [1.0, np.nan], None, 4, -32)]   # a NaN bound compares false
        for field, val, code in bad_set:
            s = M.LeastSquaresSettings(dt)
            setattr(s, field, val)
            rows.append((good, lo, up, s, 4, code))
        # the order: the guess before the bounds before the settings
        rows += [([np.nan, 5.0], lo, up, worst(), 4, -31), (good, lo, up, worst(), 0, -31), ([0.0, 5.0], lo, up, worst(), 4, -32),
                 ([np.inf, 0.0], [3.0, 3.0], up, None, 4, -31), (good, lo, up, worst(), 4, -30)]
        for x, l, u, s, m, code in rows:
            assert _raw_solve(dt, x, l, u, settings=s, m=m) == code, (dt, x, l, u, m, code)
            assert _raw(dt, x, l, u, settings=s, m=m) == code, (dt, x, l, u, m, code)


def test_python_layer_raises_the_validation_status():
    def f(x, y):
        raise AssertionError("not evaluated")
    for x, l, u, st in (([np.nan, 0.0], None, None, M.LeastSquaresStatus.badGuess), ([3.0, 0.0], [0, 0], [1, 1], M.LeastSquaresStatus.badBounds)):
        try:
            M.covariance(f, 4, x, l, u)
        except M.LeastSquaresException as e:
            assert e.status == st
        else:
            raise AssertionError("no exception")


def test_spd_inverse_argument_checks():
    L = api.lib()
    one = C.c_void_p(64)           # never dereferenced: the checks come first
    for suf in ("d", "s"):
        fn = getattr(L, "mir_lsq_spd_inverse_" + suf)
        assert fn(0, one, None, one, one, None) == -1
        assert fn(4, None, None, one, one, None) == -1 and fn(4, one, None, None, one, None) == -1 and fn(4, one, None, one, None, None) == -1
        assert fn(1 << 20, one, None, one, one, None) == -1              # beyond the column kernel's LDS vector
        fw = getattr(L, "mir_lsq_spd_inverse_work_" + suf)
        assert fw(0, one, None, one, one, one, 1 << 20, None) == -1 and fw(4, one, None, one, one, None, 1 << 20, None) == -1
        assert fw(4, one, None, one, one, one, 8, None) == -1            # scratch too small
