"""Per-problem bounds on the batched fits, CPU tier (no device needed): the flag MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM is in the
header and exported by the Python package, no struct grew and no symbol was added, optimizeLeastSquaresBatched and
optimizeLeastSquaresBatched16 validate the shapes of l / u and route 2-D bounds to the entries that take extras (1-D bounds make
the call they always made), every entry that takes extras answers 0 to count = 0 and -2 without a device after the same
argument checks, with the flag set -- and the example of tests/user_model/ compiles for gfx950 against the public header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_PROBLEM = 2
# (entry, model, n, takes a covariance)
ENTRIES = [("mir_optimize_least_squares_batched_ex_s", 0, 3, True), ("mir_optimize_least_squares_batched_ex_d", 0, 3, True),
           ("mir_lsq_batched_kernel_ex_s", 2, 8, True), ("mir_lsq_batched_kernel_ex_d", 2, 8, True),
           ("mir_lsq_batched_covariance_s", 0, 3, True), ("mir_lsq_batched_covariance_d", 0, 3, True),
           ("mir_optimize_least_squares_batched16_d", 16, 16, False), ("mir_lsq_batched16_kernel_d", 17, 11, False),
           ("mir_optimize_least_squares_batched16_ex_d", 16, 16, True), ("mir_lsq_batched16_kernel_ex_d", 17, 11, True),
           ("mir_lsq_batched16_covariance_d", 16, 16, True)]


def test_the_flag_is_in_the_header_and_exported_and_nothing_grew():
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    assert "MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM = 2u" in header
    assert M.BATCHED_BOUNDS_PER_PROBLEM == api.BATCHED_BOUNDS_PER_PROBLEM == PER_PROBLEM
    assert "BATCHED_BOUNDS_PER_PROBLEM" in api.__all__
    assert M.BATCHED_BOUNDS_PER_PROBLEM != M.BATCHED_ABSOLUTE_SIGMA
    assert C.sizeof(api.BatchedExtras) == 32 and C.sizeof(api.BatchedOptions) == 40
    assert "l_j == u_j" in header[header.index("typedef struct mir_lsq_batched_options"):header.index("typedef struct mir_lsq_batched_extras")]
    assert not re.search(r"\bint\s+mir_\w*(per_problem|problem_bounds)\w*\(", header)          # no new entry: the flag travels in the extras


def _args(name, n, count=4, m=16):
    dtype = np.float32 if name.endswith("_s") else np.float64
    R = api._Rs if dtype == np.float32 else api._Rd
    x = np.zeros((count, n), dtype); lo = np.full((count, n), -1.0, dtype); up = np.full((count, n), 1.0, dtype)
    t = np.linspace(0, 1, m, dtype=dtype); d = np.zeros((count, m), dtype); cov = np.zeros((count, n, n), dtype)
    raw = (R * count)()
    return dtype, x, lo, up, t, d, raw, cov


@pytest.mark.parametrize("name, model, n, takes_cov", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_entries_take_the_flag_in_their_argument_checks(name, model, n, takes_cov):
    """count = 0 with the flag set returns 0; without a device a call with problems answers -2 after the same argument checks
    (-1 for a missing pointer, an unknown model, a bad t_stride, an implausible struct_size), which keep their order; an extras
    that carries only the flag is valid"""
    fn = getattr(api.lib(), name)
    dtype, x, lo, up, t, d, raw, cov = _args(name, n)
    s = M.LeastSquaresSettings(dtype)
    p = lambda a: a.ctypes.data
    needs_cov = "covariance" in name
    ex = api.BatchedExtras(flags=PER_PROBLEM, covariance=p(cov) if needs_cov else None)
    good = [C.byref(s), 4, 16, model, p(x), p(lo), p(up), p(t), 0, p(d), raw, None, C.byref(ex)]
    none = list(good); none[1] = 0
    assert fn(*none) == 0
    for k in (0, 4, 5, 6, 7, 9, 10):                           # every pointer, one at a time: before the device is looked for
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    bad = list(good); bad[3] = 99
    assert fn(*bad) == -1
    bad = list(good); bad[8] = 5
    assert fn(*bad) == -1
    e2 = api.BatchedExtras(flags=PER_PROBLEM, covariance=p(cov) if needs_cov else None)
    e2.struct_size = 3
    assert fn(*(good[:12] + [C.byref(e2)])) == -1
    if not takes_cov:                                          # the batched16 entries without _ex: the flag passes, a covariance does not
        assert fn(*(good[:12] + [C.byref(api.BatchedExtras(flags=PER_PROBLEM, covariance=p(cov)))])) == -1
    if M.device_count() == 0:
        assert fn(*good) == -2


class Spy:
    def __init__(self, name, seen):
        self.name, self.seen = name, seen

    def __call__(self, *a):
        self.seen.append((self.name, a))
        return 0


def test_python_routes_two_dimensional_bounds_to_the_entries_with_extras(monkeypatch):
    L = api.lib()
    seen = []
    names = (["mir_optimize_least_squares_batched" + mid + suf for mid in ("_", "_ex_") for suf in ("s", "d")]
             + ["mir_optimize_least_squares_batched16_d", "mir_optimize_least_squares_batched16_ex_d"])
    for name in names:
        monkeypatch.setattr(L, name, Spy(name, seen))
    x = np.ones((2, 3)); t = np.linspace(0, 1, 8); d = np.zeros((2, 8))
    lo1, up1 = np.zeros(3), np.full(3, 2.0)
    lo2, up2 = np.zeros((2, 3)), np.array([[2.0, 2.0, 2.0], [3.0, 3.0, 1.0]])
    for dtype, suf in ((np.float32, "s"), (np.float64, "d")):
        M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, l=lo1, u=up1, dtype=dtype)            # today's call
        assert seen[-1][0] == "mir_optimize_least_squares_batched_" + suf and len(seen[-1][1]) == 12
        M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, l=lo1, u=up1, dtype=dtype, covariance=True)
        assert seen[-1][0].endswith("_ex_" + suf) and seen[-1][1][12]._obj.flags == 0
        out = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, l=lo2, u=up2, dtype=dtype)
        name, a = seen[-1]
        ex = a[12]._obj
        assert len(out) == 2 and name == "mir_optimize_least_squares_batched_ex_" + suf
        assert ex.flags == PER_PROBLEM and ex.struct_size == 32 and not ex.weights and not ex.covariance
        # the arrays handed over hold count x n values of the entry's type
        got = np.ctypeslib.as_array(C.cast(a[6], C.POINTER(C.c_float if suf == "s" else C.c_double)), shape=(2, 3))
        assert np.array_equal(got, up2.astype(dtype))
        for l, u in ((None, up2), (lo2, None)):                # a None beside a 2-D partner: -inf / +inf of that shape
            M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, l=l, u=u, dtype=dtype)
            a = seen[-1][1]
            assert a[12]._obj.flags == PER_PROBLEM
            k = 5 if l is None else 6
            got = np.ctypeslib.as_array(C.cast(a[k], C.POINTER(C.c_float if suf == "s" else C.c_double)), shape=(2, 3))
            assert np.all(got == (-np.inf if l is None else np.inf))
        out = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, l=lo2, u=up2, dtype=dtype, covariance=True, absolute_sigma=True)
        assert len(out) == 3 and seen[-1][1][12]._obj.flags == PER_PROBLEM | M.BATCHED_ABSOLUTE_SIGMA
    # the 16-lane models
    x16 = np.ones((2, 16)); lo16 = np.full((2, 16), -1.0); up16 = np.full((2, 16), 3.0)
    for call in (M.optimizeLeastSquaresBatched, M.optimizeLeastSquaresBatched16):
        kw = dict(dtype=np.float64) if call is M.optimizeLeastSquaresBatched else {}
        call(M.MODEL16_EXP_HARM16, x16, t, d, l=lo16[0], u=up16[0], **kw)                               # today's call: no extras
        assert seen[-1][0] == "mir_optimize_least_squares_batched16_d" and seen[-1][1][12] is None
        call(M.MODEL16_EXP_HARM16, x16, t, d, l=lo16, u=up16, **kw)                                     # its own entry, flags only
        ex = seen[-1][1][12]._obj
        assert seen[-1][0] == "mir_optimize_least_squares_batched16_d"
        assert ex.flags == PER_PROBLEM and ex.struct_size == 32 and not ex.weights and not ex.covariance
    out = M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x16, t, d, l=lo16, u=up16, weights=np.ones(8), covariance=True)
    ex = seen[-1][1][12]._obj
    assert len(out) == 3 and seen[-1][0] == "mir_optimize_least_squares_batched16_ex_d" and ex.flags == PER_PROBLEM and ex.weights
    M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x16, t, d, l=lo16[0], u=up16[0], covariance=True)
    assert seen[-1][1][12]._obj.flags == 0


def test_python_refuses_other_shapes(monkeypatch):
    L = api.lib()
    seen = []
    for name in ("mir_optimize_least_squares_batched_s", "mir_optimize_least_squares_batched_ex_s",
                 "mir_optimize_least_squares_batched16_d", "mir_optimize_least_squares_batched16_ex_d"):
        monkeypatch.setattr(L, name, Spy(name, seen))
    x = np.ones((2, 3)); t = np.linspace(0, 1, 8); d = np.zeros((2, 8))
    bad = [dict(l=np.zeros(2)), dict(u=np.zeros((3, 3))), dict(l=np.zeros((2, 3)), u=np.ones(3)), dict(l=np.zeros(3), u=np.ones((2, 3))),
           dict(l=np.zeros((2, 3, 1)), u=np.ones((2, 3, 1))), dict(l=np.zeros((1, 3)), u=np.ones((1, 3))), dict(l=0.0, u=1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, **kw)
    x16 = np.ones((2, 16))
    for kw in (dict(l=np.zeros(15)), dict(l=np.zeros((2, 16)), u=np.ones(16)), dict(u=np.ones((3, 16)))):
        with pytest.raises(ValueError):
            M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x16, t, d, **kw)
        with pytest.raises(ValueError):
            M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x16, t, d, covariance=True, **kw)
        with pytest.raises(ValueError):
            M.optimizeLeastSquaresBatched(M.MODEL16_EXP_HARM16, x16, t, d, dtype=np.float64, **kw)
    assert seen == []                                          # nothing reached a C entry


def test_the_example_builds_against_the_public_header_and_exports_its_entries():
    path = hipbuild.user_model_problem_bounds_lib()            # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    L = C.CDLL(path)
    for name in ("user_fit_peak_window_s", "user_fit_peak_window_d"):
        assert getattr(L, name)
    blob = open(path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"k_lm_batched" in blob and b"k_batched_covariance" in blob and b"PeakOnBaseline" in blob
    src = open(hipbuild.user_model_problem_bounds_paths()[0]).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["mir_optim_amd_batched.hpp"]      # the public header only
    assert "launch_batched_bounded" in src and "MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM" in src
