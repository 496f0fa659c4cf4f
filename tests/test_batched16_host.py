"""The host layer of the batched fit for models with 9 to 16 parameters (mir_optimize_least_squares_batched16_d,
mir_lsq_batched16_kernel_d, mir_lsq_batched16_jtj_d), CPU tier (no device needed): the entries are exported and declared,
their argument checks answer -1 before a device is looked for -- the model id first (0, 1 and 2 belong to the n <= 8 entries),
then the options and the extras (weights and covariance are not part of this entry yet), then the pointers and t_stride --,
`count = 0` is answered without a device, the Python wrapper refuses what the entry does not have, and a caller's own models
of 9 and 13 parameters compile against the public device header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mir_lsq_batched16_kernel_d", "mir_optimize_least_squares_batched16_d"]
N, COUNT, ROWS = 16, 4, 40


def test_entries_are_exported_and_declared():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    for name in ENTRIES + ["mir_lsq_batched16_jtj_d"]:
        assert getattr(L, name)
        assert re.search(r"\bint\s+" + name + r"\(", header), name
    assert M.MODEL16_EXP_HARM16 == 16 and M.MODEL16_GAUSS3_AFFINE == 17
    assert re.search(r"MIR_LSQ_MODEL16_EXP_HARM16\s*=\s*16\b", header) and re.search(r"MIR_LSQ_MODEL16_GAUSS3_AFFINE\s*=\s*17\b", header)
    device_header = open(os.path.join(ROOT, "include", "mir_optim_amd_batched.hpp")).read()
    assert "launch_batched16" in device_header and "batched16_lds_bytes" in device_header


def _good(n=N, count=COUNT, m=ROWS):
    s = M.LeastSquaresSettings(np.float64)
    x = np.zeros((count, n)); lo = np.full(n, -np.inf); up = np.full(n, np.inf)
    t = np.linspace(0, 1, m); d = np.zeros((count, m))
    raw = (api._Rd * max(count, 1))()
    keep = (s, x, lo, up, t, d, raw)
    p = lambda a: a.ctypes.data
    return [C.byref(s), count, m, M.MODEL16_EXP_HARM16, p(x), p(lo), p(up), p(t), 0, p(d), raw, None, None], keep


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_need_no_device(entry):
    fn = getattr(api.lib(), entry)
    good, keep = _good()
    for model in (-1, 0, 1, 2, 3, 15, 18, 99):                 # an unknown model: the ids of the n <= 8 entries included
        bad = list(good); bad[3] = model
        assert fn(*bad) == -1, model
    w = np.ones(ROWS); cov = np.zeros((COUNT, N, N))
    for ex in (api.BatchedExtras(weights=w.ctypes.data), api.BatchedExtras(covariance=cov.ctypes.data),
               api.BatchedExtras(weights=w.ctypes.data, covariance=cov.ctypes.data)):
        bad = list(good); bad[12] = C.byref(ex)
        assert fn(*bad) == -1
    stale = api.BatchedExtras(); stale.struct_size = 3          # not a struct size
    bad = list(good); bad[12] = C.byref(stale)
    assert fn(*bad) == -1
    stale = api.BatchedOptions(); stale.struct_size = 3
    bad = list(good); bad[11] = C.byref(stale)
    assert fn(*bad) == -1
    for k in (0, 4, 5, 6, 7, 9, 10):                            # every pointer, one at a time
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    for stride in (1, ROWS - 1, ROWS + 1, 2 * ROWS):            # t_stride must be 0 or m
        bad = list(good); bad[8] = stride
        assert fn(*bad) == -1, stride


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("model", [16, 17])
def test_no_problems_is_answered_without_a_device(entry, model):
    fn = getattr(api.lib(), entry)
    good, keep = _good(n=16 if model == 16 else 11)
    good[1] = 0; good[3] = model
    assert fn(*good) == 0
    good[12] = C.byref(api.BatchedExtras())                     # extras that ask for nothing are as good as none
    assert fn(*good) == 0
    good[2] = 5000                                              # ... whatever m is
    assert fn(*good) == 0


def test_the_n8_entries_keep_rejecting_the_new_ids():
    L = api.lib()
    good, keep = _good()
    for name in ("mir_lsq_batched_kernel_d", "mir_optimize_least_squares_batched_d"):
        for model in (16, 17):
            a = list(good[:12]); a[3] = model
            assert getattr(L, name)(*a) == -1, (name, model)


def test_jtj_entry_argument_checks():
    jtj = api.lib().mir_lsq_batched16_jtj_d
    J = np.zeros((2, 8, 9)); y = np.zeros((2, 8)); JJ = np.zeros((2, 16, 16)); Jy = np.zeros((2, 16))
    p = lambda a: a.ctypes.data
    assert jtj(2, 8, 17, p(J), p(y), p(JJ), p(Jy), None) == -1       # n <= 16
    assert jtj(2, 8, 0, p(J), p(y), p(JJ), p(Jy), None) == -1
    assert jtj(2, 8, 9, None, p(y), p(JJ), p(Jy), None) == -1
    assert jtj(2, 8, 9, p(J), p(y), p(JJ), None, None) == -1
    assert jtj(0, 8, 9, p(J), p(y), p(JJ), p(Jy), None) == 0         # nothing to do
    assert jtj(2, 0, 9, p(J), p(y), p(JJ), p(Jy), None) == -3
    assert jtj(2, 100000, 9, p(J), p(y), p(JJ), p(Jy), None) == -3   # beyond one workgroup's LDS


def test_python_wrapper_refuses_what_the_entry_does_not_have(monkeypatch):
    L = api.lib()
    seen = []

    def spy(*a):
        seen.append(a)
        return 0
    monkeypatch.setattr(L, "mir_optimize_least_squares_batched16_d", spy)
    x = np.ones((2, 16)); t = np.linspace(0, 4, 40); d = np.zeros((2, 40))
    for model in (M.MODEL16_EXP_HARM16, M.MODEL16_GAUSS3_AFFINE):
        with pytest.raises(ValueError):
            M.optimizeLeastSquaresBatched(model, x, t, d)                                  # the default dtype is float32
        with pytest.raises(ValueError):
            M.optimizeLeastSquaresBatched(model, x, t, d, dtype=np.float32)
        with pytest.raises(ValueError):
            M.optimizeLeastSquaresBatched(model, x, t, d, dtype=np.float64, weights=np.ones(40))
        with pytest.raises(ValueError):
            M.optimizeLeastSquaresBatched(model, x, t, d, dtype=np.float64, covariance=True)
    assert not seen
    res, xo = M.optimizeLeastSquaresBatched(M.MODEL16_EXP_HARM16, x, t, d, dtype=np.float64)
    assert len(seen) == 1 and seen[0][3] == 16 and seen[0][1] == 2 and seen[0][2] == 40 and seen[0][12] is None
    assert xo.dtype == np.float64 and len(res) == 2


def test_an_example_is_rebuilt_for_a_header_it_includes_and_for_nothing_else(monkeypatch):
    """staleness comes from the compiler's record of what the example includes: solve_wave16.h reaches user_model_n16.hip only
    through the public header and batched16_kernel.h; driver.h is the library's own"""
    lib = hipbuild.user_model_n16_lib()         # up to date from here on
    src = open(hipbuild.user_model_n16_paths()[0]).read()
    assert "solve_wave16.h" not in src and "driver.h" not in src
    ran = []
    monkeypatch.setattr(hipbuild, "_run", lambda cmd, verbose, cwd=None: ran.append(cmd))
    assert hipbuild.user_model_n16_lib() == lib and ran == []
    newer = os.path.getmtime(lib) + 10

    def touched(header):
        path = os.path.join(hipbuild.CSRC, header)
        st = os.stat(path)
        os.utime(path, (newer, newer))
        try:
            hipbuild.user_model_n16_lib()
        finally:
            os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))
        out, ran[:] = [c for c in ran if any(a.endswith("user_model_n16.hip") for a in c)], []
        return out
    assert len(touched("solve_wave16.h")) == 1
    assert touched("driver.h") == []
    assert hipbuild.user_model_n16_lib() == lib and ran == []


def test_n16_user_models_build_against_the_public_header_and_export_their_entries():
    path = hipbuild.user_model_n16_lib()        # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    L = C.CDLL(path)
    assert L.user_fit_harm9_d and L.user_fit_harm13_d and L.user_harm16_residual_d
    blob = open(path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"k_lm_batched16" in blob and b"HarmILi9" in blob and b"HarmILi13" in blob
