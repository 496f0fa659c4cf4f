"""The host layer of the batched one-wavefront-per-problem fit in both precisions, CPU tier (no device needed): the six
entries are exported and declared, their argument checks answer -1 without touching a device (the same checks in the same
order for float and double), the Python `dtype` argument routes to the f64 ones, and a caller's own double model compiles
against the public device header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mir_optimize_least_squares_batched_s", "mir_lsq_batched_kernel_s", "mir_lsq_batched_posvx_s",
           "mir_optimize_least_squares_batched_d", "mir_lsq_batched_kernel_d", "mir_lsq_batched_posvx_d")
PRECISIONS = [pytest.param("_s", np.float32, api._Rs, id="f32"), pytest.param("_d", np.float64, api._Rd, id="f64")]


def test_entries_are_exported_and_declared():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    for name in SYMBOLS:
        assert getattr(L, name)
        assert re.search(r"\bint\s+" + name + r"\(", header), name
    assert L.mir_lsq_version().decode().startswith("mir_optim_amd 0.4")


def _args(dtype, R, count=4, m=16, n=3):
    x = np.zeros((count, n), dtype); lo = np.full(n, -np.inf, dtype); up = np.full(n, np.inf, dtype)
    t = np.linspace(0, 1, m, dtype=dtype); d = np.zeros((count, m), dtype)
    raw = (R * max(count, 1))()
    return x, lo, up, t, d, raw


@pytest.mark.parametrize("suffix, dtype, R", PRECISIONS)
@pytest.mark.parametrize("entry", ["mir_lsq_batched_kernel", "mir_optimize_least_squares_batched"])
def test_argument_checks_need_no_device(entry, suffix, dtype, R):
    L = api.lib()
    fn = getattr(L, entry + suffix)
    s = M.LeastSquaresSettings(dtype)
    x, lo, up, t, d, raw = _args(dtype, R)
    p = lambda a: a.ctypes.data
    good = [C.byref(s), 4, 16, M.MODEL_EXP_DECAY, p(x), p(lo), p(up), p(t), 0, p(d), raw, None]
    for k in (0, 4, 5, 6, 7, 9, 10):                           # every pointer, one at a time
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    for model in (-1, 3, 99):                                  # an unknown model
        bad = list(good); bad[3] = model
        assert fn(*bad) == -1, model
    for stride in (1, 15, 17, 32):                             # t_stride must be 0 or m
        bad = list(good); bad[8] = stride
        assert fn(*bad) == -1, stride
    stale = api.BatchedOptions()
    stale.struct_size = 3                                      # what a 0.1 caller's stream handle looks like
    assert fn(*(good[:11] + [C.byref(stale)])) == -1


@pytest.mark.parametrize("suffix, dtype, R", PRECISIONS)
def test_posvx_argument_checks_need_no_device(suffix, dtype, R):
    posvx = getattr(api.lib(), "mir_lsq_batched_posvx" + suffix)
    P = np.zeros((2, 64), dtype); b = np.zeros((2, 8), dtype); x = np.zeros((2, 8), dtype); info = np.zeros(2, dtype=np.int32)
    p = lambda a: a.ctypes.data
    assert posvx(2, 4, p(P), p(b), p(x), p(info), None) == -1      # n is 3 or 8
    assert posvx(2, 8, None, p(b), p(x), p(info), None) == -1
    assert posvx(2, 3, p(P), p(b), None, p(info), None) == -1
    assert posvx(0, 8, p(P), p(b), p(x), p(info), None) == 0      # nothing to do


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_entry_with_no_problems_returns_nothing(dtype):
    x = np.zeros((0, 8)); t = np.linspace(0, 1, 32); d = np.zeros((0, 32))
    res, xo = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY_PAD8, x, t, d, dtype=dtype)
    assert res == [] and xo.dtype == dtype and xo.shape == (0, 8)


@pytest.mark.parametrize("fields, code", P.BAD_SETTINGS)
def test_settings_validation_codes_of_the_general_entries(fields, code):
    """The settings checks of least_squares.d:934-943 are one helper for every entry; the general ones answer before they look
    for a device (the batched host entry looks for the device first: its codes are compared in tests/test_gpu_batched.py)."""
    def f(x, y):
        y[:] = x
    for dtype in (np.float32, np.float64):
        s = M.LeastSquaresSettings(dtype)
        for name, value in fields.items():
            setattr(s, name, value)
        res, _ = M.optimizeLeastSquares(f, 2, [0.5, 0.5], settings=s, dtype=dtype)
        assert res.status == M.LeastSquaresStatus[code], (dtype, res)
        assert res.iterations == 0 and res.fCalls == 0 and res.residual == np.inf


def test_python_dtype_routes_to_the_f64_entries(monkeypatch):
    """dtype=np.float64 calls the _d entries with double arrays and the _d settings; the default stays float32 (_s)."""
    L = api.lib()
    seen = []

    class Spy:
        def __init__(self, name):
            self.name = name

        def __call__(self, *a):
            seen.append((self.name, a))
            return 0
    for name in ("mir_optimize_least_squares_batched_s", "mir_optimize_least_squares_batched_d"):
        monkeypatch.setattr(L, name, Spy(name))
    x = np.ones((2, 3)); t = np.linspace(0, 1, 8); d = np.zeros((2, 8))
    res, xo = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, dtype=np.float64)
    assert seen[-1][0] == "mir_optimize_least_squares_batched_d" and xo.dtype == np.float64
    assert isinstance(seen[-1][1][0]._obj, api._Sd) and isinstance(seen[-1][1][10][0], api._Rd)
    res, xo = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d)
    assert seen[-1][0] == "mir_optimize_least_squares_batched_s" and xo.dtype == np.float32
    assert isinstance(seen[-1][1][0]._obj, api._Ss) and isinstance(seen[-1][1][10][0], api._Rs)
    with pytest.raises(ValueError):
        M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, dtype=np.float16)
    with pytest.raises(ValueError):
        M.batchedPosvx(np.eye(3)[None], np.ones((1, 3)), dtype=np.int32)


def test_f64_user_model_builds_against_the_public_header_and_exports_its_entries():
    path = hipbuild.user_model_f64_lib()        # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    L = C.CDLL(path)
    assert L.user_fit_damped_cosine_d and L.user_pad8_residual_d
    # ... and it really is the gfx950 code object of a double model: its kernel is in the library
    blob = open(path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"DampedCosineD" in blob
