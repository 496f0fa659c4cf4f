"""MIR_LSQ_BATCHED_DEVICE_BOUNDS (bounded steps solved inside the batched wave kernel), CPU tier: the constant of the Python
layer is the header's, the bit changes nothing about the entries' argument checks or what they answer without a device, the
options struct and the exported symbols are what they were, and a caller's model compiles against launch_batched_bounded while
a caller of launch_batched alone gets no bounded kernel. The fits themselves: tests/test_gpu_batched_bounds.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [pytest.param("_s", np.float32, api._Rs, id="f32"), pytest.param("_d", np.float64, api._Rd, id="f64")]
ENTRIES = ["mir_lsq_batched_kernel", "mir_optimize_least_squares_batched", "mir_lsq_batched_kernel_ex",
           "mir_optimize_least_squares_batched_ex"]


def test_python_constant_is_the_headers_and_the_bit_is_free():
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    value = int(re.search(r"enum\s*\{\s*MIR_LSQ_BATCHED_DEVICE_BOUNDS\s*=\s*(\d+)\s*\}", header).group(1))
    assert M.BATCHED_DEVICE_BOUNDS == api.BATCHED_DEVICE_BOUNDS == value == 4
    assert "BATCHED_DEVICE_BOUNDS" in api.__all__
    others = {name: int(v) for name, v in re.findall(r"enum\s*\{\s*(MIR_LSQ_BATCHED_(?:NO_LADDER|ANALYTIC_JACOBIAN))\s*=\s*(\d+)\s*\}", header)}
    assert others == {"MIR_LSQ_BATCHED_NO_LADDER": 1, "MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN": 2}
    assert all(value & v == 0 for v in others.values())
    assert M.BATCHED_NO_LADDER == 1


def test_no_new_symbol_no_larger_options_same_version():
    L = api.lib()
    assert C.sizeof(api.BatchedOptions) == 40
    assert L.mir_lsq_version().decode().startswith("mir_optim_amd 0.4")
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    assert not re.search(r"\bmir_\w*bounded\w*\s*\(", header)           # the switch is a variant bit, not an entry


@pytest.mark.parametrize("suffix, dtype, R", PRECISIONS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_bit_changes_no_answer_that_needs_no_device(entry, suffix, dtype, R):
    fn = getattr(api.lib(), entry + suffix)
    s = M.LeastSquaresSettings(dtype)
    count, m, n = 4, 16, 3
    x = np.ones((count, n), dtype); lo = np.full(n, -np.inf, dtype); up = np.full(n, np.inf, dtype)
    t = np.linspace(0, 1, m, dtype=dtype); d = np.zeros((count, m), dtype)
    raw = (R * count)()
    p = lambda a: a.ctypes.data
    ex = [None] if entry.endswith("_ex") else []

    def call(variant, **change):
        args = [C.byref(s), count, m, M.MODEL_EXP_DECAY, p(x), p(lo), p(up), p(t), 0, p(d), raw,
                C.byref(api.BatchedOptions(variant=variant))] + ex
        for k, v in change.items():
            args[int(k[1:])] = v
        return fn(*args)
    for change in ({"a4": None}, {"a5": None}, {"a7": None}, {"a9": None}, {"a10": None}, {"a3": 7}, {"a8": 5}):
        assert call(M.BATCHED_DEVICE_BOUNDS, **change) == call(0, **change) == -1, change
    assert call(M.BATCHED_DEVICE_BOUNDS, a1=0) == call(0, a1=0) == 0        # no problems: nothing to launch
    if M.device_count() == 0:
        assert call(M.BATCHED_DEVICE_BOUNDS) == call(0) == -2
        assert call(M.BATCHED_DEVICE_BOUNDS | M.BATCHED_NO_LADDER) == -2


def test_bounded_user_model_builds_against_the_public_header():
    path = hipbuild.user_model_bounded_lib()        # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    L = C.CDLL(path)
    assert L.user_fit_logistic_bounded_d and L.user_fit_logistic_bounded_s and L.user_fit_logistic_d
    blob = open(path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"LogisticGrowth" in blob and b"BatchedBoxQpStep" in blob


def test_a_caller_of_launch_batched_alone_gets_no_bounded_kernel():
    """launch_batched<Model> instantiates what it always did: the three earlier example libraries hold no bounded instance"""
    hipbuild.build_user_model_example()
    d = os.path.join(ROOT, "tests", "user_model")
    for name in ("libuser_model.so", "libuser_model_f64.so", "libuser_model_weighted.so"):
        assert b"BatchedBoxQpStep" not in open(os.path.join(d, name), "rb").read(), name
