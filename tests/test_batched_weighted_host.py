"""Per-row weights and parameter covariance on the batched path, CPU tier (no device needed): the six new entries
(mir_optimize_least_squares_batched_ex_s/_d, mir_lsq_batched_kernel_ex_s/_d, mir_lsq_batched_covariance_s/_d) are exported
and declared, their argument checks answer -1 before they look for a device, count = 0 returns 0, the Python keywords
`weights`, `covariance` and `absolute_sigma` route to the _ex entries while a plain call still calls the old ones, the weighted
user model compiles for gfx950 against the public header -- and the problem set of the GPU tier is what its docstring says:
the f64 oracle converges on all 64 weighted EXP_DECAY problems and its weighted minimiser differs from the unweighted one
beyond rtol 1e-6 on every one of them (a fit that ignored the weights could not pass the comparison)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import weighted_problems as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mir_optimize_least_squares_batched_ex_s", "mir_optimize_least_squares_batched_ex_d", "mir_lsq_batched_kernel_ex_s",
           "mir_lsq_batched_kernel_ex_d", "mir_lsq_batched_covariance_s", "mir_lsq_batched_covariance_d")
PRECISIONS = [pytest.param("_s", np.float32, api._Rs, id="f32"), pytest.param("_d", np.float64, api._Rd, id="f64")]
ENTRIES = ["mir_optimize_least_squares_batched_ex", "mir_lsq_batched_kernel_ex", "mir_lsq_batched_covariance"]


def test_entries_are_exported_and_declared():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    for name in SYMBOLS:
        assert getattr(L, name)
        assert re.search(r"\bint\s+" + name + r"\(", header), name
    assert re.search(r"typedef struct mir_lsq_batched_extras\s*\{", header) and "MIR_LSQ_BATCHED_ABSOLUTE_SIGMA = 1u" in header
    assert C.sizeof(api.BatchedExtras) == 32 and C.sizeof(api.BatchedOptions) == 40     # the options did not grow
    assert api.BatchedExtras.weights.offset == 8 and api.BatchedExtras.weight_stride.offset == 16
    assert api.BatchedExtras.covariance.offset == 24
    assert L.mir_lsq_version().decode().startswith("mir_optim_amd 0.4")                  # callers discover the symbols by name


def _args(dtype, R, count=4, m=16, n=3):
    x = np.zeros((count, n), dtype); lo = np.full(n, -np.inf, dtype); up = np.full(n, np.inf, dtype)
    t = np.linspace(0, 1, m, dtype=dtype); d = np.zeros((count, m), dtype)
    w = np.ones((count, m), dtype); cov = np.zeros((count, n, n), dtype)
    raw = (R * max(count, 1))()
    return x, lo, up, t, d, raw, w, cov


@pytest.mark.parametrize("suffix, dtype, R", PRECISIONS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_need_no_device(entry, suffix, dtype, R):
    fn = getattr(api.lib(), entry + suffix)
    s = M.LeastSquaresSettings(dtype)
    x, lo, up, t, d, raw, w, cov = _args(dtype, R)
    p = lambda a: a.ctypes.data
    ex = api.BatchedExtras(weights=p(w), weight_stride=16, covariance=p(cov))
    good = [C.byref(s), 4, 16, M.MODEL_EXP_DECAY, p(x), p(lo), p(up), p(t), 0, p(d), raw, None, C.byref(ex)]
    for k in (0, 4, 5, 6, 7, 9, 10):                           # every pointer, one at a time
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    for model in (-1, 3, 99):                                  # an unknown model
        bad = list(good); bad[3] = model
        assert fn(*bad) == -1, model
    for stride in (1, 15, 17, 32):                             # t_stride must be 0 or m
        bad = list(good); bad[8] = stride
        assert fn(*bad) == -1, stride
    for stride in (1, 15, 17, 32, 64):                         # weight_stride must be 0 or m
        e2 = api.BatchedExtras(weights=p(w), weight_stride=stride, covariance=p(cov))
        assert fn(*(good[:12] + [C.byref(e2)])) == -1, stride
    for size in (0, 3, 7, 4096, 0xFFFFFFFF):                   # an implausible struct_size
        e2 = api.BatchedExtras(weights=p(w), weight_stride=16, covariance=p(cov))
        e2.struct_size = size
        assert fn(*(good[:12] + [C.byref(e2)])) == -1, size
    stale = api.BatchedOptions()
    stale.struct_size = 3                                      # the options check of the existing entries is still there
    assert fn(*(good[:11] + [C.byref(stale), C.byref(ex)])) == -1
    if entry == "mir_lsq_batched_covariance":                  # there the extras and their covariance are the point of the call
        assert fn(*(good[:12] + [None])) == -1
        assert fn(*(good[:12] + [C.byref(api.BatchedExtras(weights=p(w), weight_stride=16))])) == -1


@pytest.mark.parametrize("suffix, dtype, R", PRECISIONS)
def test_host_entry_rejects_non_finite_weights(suffix, dtype, R):
    fn = getattr(api.lib(), "mir_optimize_least_squares_batched_ex" + suffix)
    s = M.LeastSquaresSettings(dtype)
    p = lambda a: a.ctypes.data
    for value in (np.nan, np.inf, -np.inf):
        for stride in (0, 16):
            x, lo, up, t, d, raw, w, cov = _args(dtype, R)
            w[0 if stride == 0 else 3, 11] = value             # stride 0 reads the first m values only
            ex = api.BatchedExtras(weights=p(w), weight_stride=stride)
            assert fn(C.byref(s), 4, 16, M.MODEL_EXP_DECAY, p(x), p(lo), p(up), p(t), 0, p(d), raw, None, C.byref(ex)) == -1
    with pytest.raises(RuntimeError, match="-1"):
        M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, np.ones((2, 3)), np.linspace(0, 1, 8), np.zeros((2, 8)),
                                      weights=np.full(8, np.nan), dtype=dtype)


@pytest.mark.parametrize("suffix, dtype, R", PRECISIONS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_no_problems_is_no_work(entry, suffix, dtype, R):
    fn = getattr(api.lib(), entry + suffix)
    s = M.LeastSquaresSettings(dtype)
    x, lo, up, t, d, raw, w, cov = _args(dtype, R)
    p = lambda a: a.ctypes.data
    ex = api.BatchedExtras(weights=p(w), weight_stride=16, covariance=p(cov))
    assert fn(C.byref(s), 0, 16, M.MODEL_EXP_DECAY, p(x), p(lo), p(up), p(t), 0, p(d), raw, None, C.byref(ex)) == 0
    if entry != "mir_lsq_batched_covariance":                  # and without extras an _ex entry is the entry it extends
        assert fn(C.byref(s), 0, 16, M.MODEL_EXP_DECAY, p(x), p(lo), p(up), p(t), 0, p(d), raw, None, None) == 0


@pytest.mark.parametrize("suffix, dtype, R", PRECISIONS)
def test_no_problems_whatever_m_is_and_the_covariance_entry_still_needs_its_output(suffix, dtype, R):
    """count = 0 is answered 0 before m is looked at (m = 10^6 fits no LDS) and without a device, by the entries with and
    without extras; the covariance entry answers -1 without extras or without a covariance even then"""
    L = api.lib()
    s = M.LeastSquaresSettings(dtype)
    x, lo, up, t, d, raw, w, cov = _args(dtype, R)
    p = lambda a: a.ctypes.data
    none = [C.byref(s), 0, 10 ** 6, M.MODEL_EXP_DECAY_PAD8, p(x), p(lo), p(up), p(t), 0, p(d), raw, None]
    for entry in ("mir_optimize_least_squares_batched", "mir_lsq_batched_kernel"):
        assert getattr(L, entry + suffix)(*none) == 0, entry
    ex = api.BatchedExtras(covariance=p(cov))
    for entry in ENTRIES:
        assert getattr(L, entry + suffix)(*(none + [C.byref(ex)])) == 0, entry
    fn = getattr(L, "mir_lsq_batched_covariance" + suffix)
    assert fn(*(none + [None])) == -1
    assert fn(*(none + [C.byref(api.BatchedExtras(weights=p(w)))])) == -1


@pytest.mark.parametrize("suffix, dtype, R", PRECISIONS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_analytic_jacobian_of_a_model_without_grad_is_refused_after_the_device_check(entry, suffix, dtype, R):
    """none of the built-in models of up to 8 parameters has grad: the launch refuses (-1 from the device-pointer entries, -5
    from the host-pointer one, which folds it into its launch) -- behind the device check, so -2 without a device"""
    fn = getattr(api.lib(), entry + suffix)
    s = M.LeastSquaresSettings(dtype)
    x, lo, up, t, d, raw, w, cov = _args(dtype, R)
    p = lambda a: a.ctypes.data
    ex = api.BatchedExtras(covariance=p(cov))
    rc = fn(C.byref(s), 4, 16, M.MODEL_EXP_DECAY, p(x), p(lo), p(up), p(t), 0, p(d), raw, C.byref(api.BatchedOptions(variant=2)), C.byref(ex))
    assert rc == (-2 if M.device_count() == 0 else -5 if entry.startswith("mir_optimize") else -1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_python_with_no_problems_returns_empty_arrays(dtype):
    x = np.zeros((0, 8)); t = np.linspace(0, 1, 32); d = np.zeros((0, 32))
    res, xo, cov = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY_PAD8, x, t, d, dtype=dtype, weights=np.ones(32), covariance=True)
    assert res == [] and xo.shape == (0, 8) and cov.shape == (0, 8, 8) and cov.dtype == dtype


def test_python_keywords_route_to_the_ex_entries(monkeypatch):
    L = api.lib()
    seen = []

    class Spy:
        def __init__(self, name):
            self.name = name

        def __call__(self, *a):
            seen.append((self.name, a))
            return 0
    names = ["mir_optimize_least_squares_batched" + mid + suf for mid in ("_", "_ex_") for suf in ("s", "d")]
    for name in names:
        monkeypatch.setattr(L, name, Spy(name))
    x = np.ones((2, 3)); t = np.linspace(0, 1, 8); d = np.zeros((2, 8)); w = np.full(8, 2.0)
    for dtype, suf in ((np.float32, "s"), (np.float64, "d")):
        out = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, dtype=dtype)
        assert len(out) == 2 and seen[-1][0] == "mir_optimize_least_squares_batched_" + suf and len(seen[-1][1]) == 12
        out = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, dtype=dtype, weights=w)
        assert len(out) == 2 and seen[-1][0] == "mir_optimize_least_squares_batched_ex_" + suf
        ex = seen[-1][1][12]._obj
        assert ex.struct_size == 32 and ex.weights and ex.weight_stride == 0 and not ex.covariance and ex.flags == 0
        out = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, dtype=dtype, weights=np.tile(w, (2, 1)), covariance=True,
                                            absolute_sigma=True)
        assert len(out) == 3 and out[2].shape == (2, 3, 3) and out[2].dtype == dtype
        ex = seen[-1][1][12]._obj
        assert seen[-1][0].endswith("_ex_" + suf) and ex.weight_stride == 8 and ex.covariance == out[2].ctypes.data
        assert ex.flags == M.BATCHED_ABSOLUTE_SIGMA == 1
        out = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, dtype=dtype, covariance=True)
        ex = seen[-1][1][12]._obj
        assert len(out) == 3 and seen[-1][0].endswith("_ex_" + suf) and not ex.weights and ex.covariance
    with pytest.raises(ValueError):
        M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x, t, d, weights=np.ones(7))


def test_weighted_user_model_builds_against_the_public_header_and_exports_its_entries():
    path = hipbuild.user_model_weighted_lib()   # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    L = C.CDLL(path)
    for name in ("user_fit_weighted_peak_s", "user_fit_weighted_peak_d", "user_weighted_peak_covariance_s",
                 "user_weighted_peak_covariance_d"):
        assert getattr(L, name)
    blob = open(path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"k_batched_covariance" in blob and b"WeightedPeak" in blob
    src = open(hipbuild.user_model_weighted_paths()[0]).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["mir_optim_amd_batched.hpp"]      # the public header only


def test_the_weighted_problem_set_cannot_be_fitted_by_ignoring_the_weights(oracle):
    count = 64
    t, data, x0, w = WP.exp_decay_weighted(count)
    assert [int(np.count_nonzero(w[k] == 0)) for k in range(8)] == [37, 0, 0, 0, 37, 0, 0, 0]
    worst_cond = 0.0
    for k in range(count):
        rw, xw = oracle.optimize(WP.weighted_f(WP.EXP_DECAY, t, data[k], w[k]), t.size, x0[k], dtype=np.float64)
        ru, xu = oracle.optimize(WP.weighted_f(WP.EXP_DECAY, t, data[k], np.ones_like(t)), t.size, x0[k], dtype=np.float64)
        assert rw.status >= 0 and ru.status >= 0, (k, rw.status, ru.status)
        assert not np.allclose(xw, xu, rtol=1e-6, atol=0), (k, xw, xu)
        J = WP.model_jacobian(WP.EXP_DECAY, t, xw) * w[k][:, None]
        worst_cond = max(worst_cond, np.linalg.cond(J.T @ J))
    assert worst_cond < 1.05e3, worst_cond              # well conditioned: 1.0e3 to two digits
