"""The fitted curve and its confidence band on the batched path (mir_lsq_batched_predict_s / _d, mir_lsq_batched16_predict_d,
launch_batched_predict<Model>, M.predictBatched), CPU tier (no device needed): the entries are exported and declared, no struct
grew, every -1 is answered before a device is looked for, one argument at a time, the wrapper's shape errors, and the example
library compiles for gfx950. The numbers are tested on the GPU (tests/test_gpu_batched_predict.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import predict_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> (dtype, a model id it takes with its n, the ids it refuses)
ENTRIES = {
    "mir_lsq_batched_predict_s": (np.float32, (M.MODEL_EXP_DECAY_PAD8, 8), (-1, 3, 15, 16, 17, 18, 99)),
    "mir_lsq_batched_predict_d": (np.float64, (M.MODEL_EXP_DECAY, 3), (-1, 3, 15, 16, 17, 18, 99)),
    "mir_lsq_batched16_predict_d": (np.float64, (M.MODEL16_EXP_HARM16, 16), (-1, 0, 1, 2, 3, 15, 18, 99)),
}
COUNT, Q = 4, 40


def test_entries_are_exported_and_declared():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    for name in ENTRIES:
        assert getattr(L, name)
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert "per_problem" not in name and "problem_bounds" not in name
        assert header.index("int " + name + "(") > header.index("int mir_lsq_batched16_jtj_d(")      # declared after it
    device_header = open(os.path.join(ROOT, "include", "mir_optim_amd_batched.hpp")).read()
    assert "launch_batched_predict" in device_header and "batched_predict.h" in device_header
    assert "predictBatched" in api.__all__ and M.predictBatched is api.predictBatched


def test_no_struct_grew_and_the_units_are_built():
    assert C.sizeof(api.BatchedExtras) == 32 and C.sizeof(api.BatchedOptions) == 40
    L = api.lib()
    assert L.mir_lsq_version().decode().startswith("mir_optim_amd 0.4")                  # callers discover the symbols by name
    assert "batched_predict.hip" in hipbuild.SOLVER_UNITS and "batched_predict_d.hip" in hipbuild.SOLVER_UNITS
    assert "user_model_predict" in hipbuild.USER_MODELS
    for dtype in (np.float32, np.float64):
        assert M.LeastSquaresSettings(dtype).jacobianEpsilon == PC.EPS[dtype]


def _good(entry, count=COUNT, q=Q, model=None):
    dtype, (mid, n), _ = ENTRIES[entry]
    s = M.LeastSquaresSettings(dtype)
    x = np.ones((count, n), dtype); lo = np.full(n, -np.inf, dtype); up = np.full(n, np.inf, dtype)
    tq = np.linspace(0, 1, max(q, 1)).astype(dtype)
    cov = np.zeros((max(count, 1), n, n), dtype); value = np.zeros((max(count, 1), max(q, 1)), dtype); sigma = value.copy()
    keep = (s, x, lo, up, tq, cov, value, sigma)
    p = lambda a: a.ctypes.data                                # noqa: E731
    #        0          1      2  3                                4     5      6      7      8  9       10        11        12    13
    return [C.byref(s), count, q, mid if model is None else model, p(x), p(lo), p(up), p(tq), 0, p(cov), p(value), p(sigma), None, None], keep


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_argument_checks_need_no_device(entry):
    fn = getattr(api.lib(), entry)
    good, keep = _good(entry)
    for model in ENTRIES[entry][2]:                             # an unknown model, the other family's ids included
        bad = list(good); bad[3] = model
        assert fn(*bad) == -1, model
    for k in (0, 4, 7, 10):                                     # settings, x, tq, value: one at a time
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    for k in (5, 6):                                            # lower without upper, upper without lower
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    bad = list(good); bad[9] = None                             # sigma without a covariance
    assert fn(*bad) == -1
    for stride in (1, Q - 1, Q + 1, 2 * Q):                     # tq_stride must be 0 or q
        bad = list(good); bad[8] = stride
        assert fn(*bad) == -1, stride
    for big in (2 ** 31, 2 ** 31 + 5, 2 ** 40):                 # count, q < 2^31
        bad = list(good); bad[1] = big
        assert fn(*bad) == -1, big
        bad = list(good); bad[2] = big
        assert fn(*bad) == -1, big
        bad[8] = big                                            # (also with the stride that would go with it)
        assert fn(*bad) == -1, big
    w = np.ones(Q, ENTRIES[entry][0])
    for ex in (api.BatchedExtras(weights=w.ctypes.data), api.BatchedExtras(covariance=keep[5].ctypes.data),
               api.BatchedExtras(flags=2, weights=w.ctypes.data, weight_stride=Q)):      # extras with weights or a covariance pointer
        bad = list(good); bad[13] = C.byref(ex)
        assert fn(*bad) == -1
    for size in (0, 3, 7, 5000):                                # not a struct size
        stale = api.BatchedExtras(); stale.struct_size = size
        bad = list(good); bad[13] = C.byref(stale)
        assert fn(*bad) == -1, size
        stale = api.BatchedOptions(); stale.struct_size = size
        bad = list(good); bad[12] = C.byref(stale)
        assert fn(*bad) == -1, size
    # the analytic Jacobian of a model without a derivative
    model = M.MODEL16_GAUSS3_AFFINE if entry.startswith("mir_lsq_batched16") else None
    g2, keep2 = (_good(entry) if model is None else _good_gauss3())
    g2[12] = C.byref(api.BatchedOptions(variant=2))
    assert fn(*g2) == -1
    # every one of them also when there is nothing to do
    bad = list(good); bad[1] = 0; bad[10] = None
    assert fn(*bad) == -1
    bad = list(good); bad[2] = 0; bad[8] = 3
    assert fn(*bad) == -1


def _good_gauss3():
    s = M.LeastSquaresSettings(np.float64)
    x = np.ones((COUNT, 11)); tq = np.linspace(0, 1, Q); value = np.zeros((COUNT, Q))
    keep = (s, x, tq, value)
    p = lambda a: a.ctypes.data                                # noqa: E731
    return [C.byref(s), COUNT, Q, M.MODEL16_GAUSS3_AFFINE, p(x), None, None, p(tq), 0, None, p(value), None, None, None], keep


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_nothing_to_do_is_answered_without_a_device(entry):
    fn = getattr(api.lib(), entry)
    good, keep = _good(entry, count=0)
    assert fn(*good) == 0
    good, keep = _good(entry, q=0)
    assert fn(*good) == 0
    good[12] = C.byref(api.BatchedOptions(variant=1)); good[13] = C.byref(api.BatchedExtras(flags=1 | 2 | 64))   # flags pass
    assert fn(*good) == 0


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_well_formed_call_without_a_device_is_answered_minus_2(entry):
    """... after every -1. (The arguments here are host arrays: with a device the call is the GPU tests' to make, and this test
    holds only that the entry is there.)"""
    fn = getattr(api.lib(), entry)
    if M.device_count() != 0:
        return
    for change in ({}, {5: None, 6: None}, {9: None, 11: None}, {8: Q}, {13: C.byref(api.BatchedExtras(flags=2))}):
        good, keep = _good(entry)
        for k, v in change.items():
            good[k] = v
        assert fn(*good) == -2, change
    if entry.startswith("mir_lsq_batched16"):
        g2, keep2 = _good_gauss3()
        assert fn(*g2) == -2
        good, keep = _good(entry)
        good[12] = C.byref(api.BatchedOptions(variant=2))       # EXP_HARM16 has a derivative
        assert fn(*good) == -2


def test_python_shape_errors():
    x = np.ones((COUNT, 3)); tq = np.linspace(0, 1, Q); cov = np.zeros((COUNT, 3, 3))
    for bad_tq in (np.zeros((COUNT + 1, Q)), np.zeros((2, COUNT, Q)), np.zeros((1, Q))):
        with pytest.raises(ValueError):
            M.predictBatched(M.MODEL_EXP_DECAY, x, bad_tq)
    for bad_cov in (np.zeros((COUNT, 3)), np.zeros((COUNT, 3, 4)), np.zeros((COUNT + 1, 3, 3)), np.zeros((3, 3))):
        with pytest.raises(ValueError):
            M.predictBatched(M.MODEL_EXP_DECAY, x, tq, bad_cov)
    for l, u in ((np.zeros(4), None), (np.zeros((COUNT, 3)), np.zeros(3)), (None, np.zeros((COUNT + 1, 3)))):
        with pytest.raises(ValueError):
            M.predictBatched(M.MODEL_EXP_DECAY, x, tq, cov, l=l, u=u)
    with pytest.raises(ValueError):
        M.predictBatched(M.MODEL_EXP_DECAY, np.ones((COUNT, 4)), tq)            # n of the model
    with pytest.raises(ValueError):
        M.predictBatched(M.MODEL_EXP_DECAY, np.ones(3), tq)
    with pytest.raises(ValueError):
        M.predictBatched(M.MODEL16_EXP_HARM16, np.ones((COUNT, 16)), tq)        # float32 by default: the 16-wide models are float64
    with pytest.raises(ValueError):
        M.predictBatched(M.MODEL_EXP_DECAY, x, tq, dtype=np.float16)
    # nothing to do needs no device
    v = M.predictBatched(M.MODEL_EXP_DECAY, np.ones((0, 3)), tq)
    assert v.shape == (0, Q)
    v, s = M.predictBatched(M.MODEL_EXP_DECAY, x, np.zeros(0), cov, dtype=np.float64)
    assert v.shape == s.shape == (COUNT, 0) and v.dtype == np.float64


def test_reference_measures_and_float_casts():
    """the inputs of the GPU cases: every covariance stays positive definite when cast to the dtype of its cases, and the
    reference's fixed-parameter and one-sided rules do what the kernel's comment says"""
    for name in ("exp_decay", "exp3", "pad8", "peak"):
        assert PC.min_eig_ratio(name, np.float32) > 0, name
    for name in ("harm13", "harm16", "gauss3"):
        assert PC.min_eig_ratio(name, np.float64) > 0, name
    fam = PC.family("exp_decay")
    tq = PC.grid(33)
    v, s, mag = PC.reference(fam, fam.x, fam.C, tq)
    assert (s > 0).all() and (s <= mag * np.sqrt(3) * (1 + 1e-12)).all()
    lo = np.full((PC.COUNT, 3), -np.inf); up = np.full((PC.COUNT, 3), np.inf)
    lo[:, 1] = up[:, 1] = fam.x[:, 1]
    v2, s2, _ = PC.reference(fam, fam.x, fam.C, tq, lo, up)
    g = fam.jacobian(tq, fam.x[0])[:, [0, 2]]
    assert np.allclose(s2[0], np.sqrt(np.einsum("ij,jk,ik->i", g, fam.C[0][np.ix_([0, 2], [0, 2])], g)), rtol=1e-13)
    assert (v2 == v).all()


def test_the_example_library_builds_for_gfx950():
    path = hipbuild.user_model_predict_lib()
    L = C.CDLL(path)
    for name in ("user_predict_peak_s", "user_predict_peak_d", "user_predict_harm13_d"):
        assert getattr(L, name)
    blob = open(path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"k_batched_predict" in blob and b"WeightedPeak" in blob and b"Harm" in blob
    src = open(hipbuild.user_model_predict_paths()[0]).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["mir_optim_amd_batched.hpp"]      # the public header only
    # no-device answers of the header's launch: -1 before anything else, 0 for nothing to do
    fn = L.user_predict_peak_d
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 5
    s = M.LeastSquaresSettings(np.float64)
    x = np.ones((COUNT, 5)); tq = np.linspace(0, 1, Q); value = np.zeros((COUNT, Q))
    p = lambda a: a.ctypes.data                                # noqa: E731
    assert fn(C.byref(s), COUNT, Q, p(x), None, None, p(tq), 1, None, p(value), None, None, None) == -1
    assert fn(C.byref(s), COUNT, Q, p(x), None, None, p(tq), 0, None, p(value), p(value), None, None) == -1
    assert fn(C.byref(s), 0, Q, p(x), None, None, p(tq), 0, None, p(value), None, None, None) == 0
    assert fn(C.byref(s), COUNT, 0, p(x), None, None, p(tq), 0, None, p(value), None, None, None) == 0
