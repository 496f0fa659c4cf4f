"""Per-row weights and parameter covariance of the batched fit for models with 9 to 16 parameters, CPU tier (no device needed):
the three entries (mir_optimize_least_squares_batched16_ex_d, mir_lsq_batched16_kernel_ex_d, mir_lsq_batched16_covariance_d)
are exported and declared and answer their argument checks before a device is looked for; M.optimizeLeastSquaresBatched16
checks dtypes and shapes and sends a call without extras to the old entry; the caller's weighted models of 9 and 13 parameters
compile against the public device header.

And the reference side of tests/test_gpu_batched16_weighted.py, with the oracle on every problem set of
tests/batched16_weighted_problems.py (SETS): every weighted fit ends with status >= 0; the weighted and the unweighted
minimisers differ beyond rtol 1e-6 on every problem (a fit that ignores its weights fails the GPU test); the oracle against
ITSELF with the rows reversed stays inside the tight bar of test_gpu_batched16.compare on at least 95 % of the problems. Each
set's largest equilibrated condition number and its covariance gap of float64 central differences (h = 2^-26) against the
analytic Jacobian are printed: the covariance bars of the GPU test are built from them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import batched16_weighted_problems as WP16
from test_gpu_batched16 import gaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_ENTRIES = ["mir_lsq_batched16_kernel_ex_d", "mir_optimize_least_squares_batched16_ex_d"]
ENTRIES = FIT_ENTRIES + ["mir_lsq_batched16_covariance_d"]
N, COUNT, ROWS = 16, 4, 40


def test_entries_are_exported_and_declared():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    for name in ENTRIES:
        assert getattr(L, name)
        assert re.search(r"\bint\s+" + name + r"\(", header), name
    device_header = open(os.path.join(ROOT, "include", "mir_optim_amd_batched.hpp")).read()
    assert "launch_batched16_covariance" in device_header
    assert "optimizeLeastSquaresBatched16" in api.__all__
    assert M.optimizeLeastSquaresBatched16 is api.optimizeLeastSquaresBatched16


def _good(n=N, count=COUNT, m=ROWS, model=M.MODEL16_EXP_HARM16):
    s = M.LeastSquaresSettings(np.float64)
    x = np.zeros((count, n)); lo = np.full(n, -np.inf); up = np.full(n, np.inf)
    t = np.linspace(0, 1, m); d = np.zeros((count, m))
    raw = (api._Rd * max(count, 1))()
    w = np.ones(m); cov = np.zeros((max(count, 1), n, n))
    ex = api.BatchedExtras(weights=w.ctypes.data, covariance=cov.ctypes.data)
    keep = (s, x, lo, up, t, d, raw, w, cov, ex)
    p = lambda a: a.ctypes.data
    return [C.byref(s), count, m, model, p(x), p(lo), p(up), p(t), 0, p(d), raw, None, C.byref(ex)], keep


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_need_no_device(entry):
    fn = getattr(api.lib(), entry)
    good, keep = _good()
    w, cov = keep[7], keep[8]
    for model in (-1, 0, 1, 2, 3, 15, 18, 99):                 # an unknown model: the ids of the n <= 8 entries included
        bad = list(good); bad[3] = model
        assert fn(*bad) == -1, model
    for size in (0, 3, 7, 5000):                                # not a struct size
        stale = api.BatchedExtras(weights=w.ctypes.data, covariance=cov.ctypes.data); stale.struct_size = size
        bad = list(good); bad[12] = C.byref(stale)
        assert fn(*bad) == -1, size
    stale = api.BatchedOptions(); stale.struct_size = 3
    bad = list(good); bad[11] = C.byref(stale)
    assert fn(*bad) == -1
    for k in (0, 4, 5, 6, 7, 9, 10):                            # every pointer, one at a time
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    for stride in (1, ROWS - 1, ROWS + 1, 2 * ROWS):            # t_stride must be 0 or m
        bad = list(good); bad[8] = stride
        assert fn(*bad) == -1, stride
    for stride in (1, ROWS - 1, ROWS + 1, 2 * ROWS):            # ... and so must the weight stride
        ex = api.BatchedExtras(weights=w.ctypes.data, weight_stride=stride, covariance=cov.ctypes.data)
        bad = list(good); bad[12] = C.byref(ex)
        assert fn(*bad) == -1, stride
    # the model without a derivative refuses the analytic Jacobian
    g11, keep11 = _good(n=11, model=M.MODEL16_GAUSS3_AFFINE)
    g11[11] = C.byref(api.BatchedOptions(variant=2))
    assert fn(*g11) == -1


def test_the_covariance_entry_needs_somewhere_to_write():
    fn = api.lib().mir_lsq_batched16_covariance_d
    good, keep = _good()
    w = keep[7]
    for ex in (None, C.byref(api.BatchedExtras()), C.byref(api.BatchedExtras(weights=w.ctypes.data))):
        bad = list(good); bad[12] = ex
        assert fn(*bad) == -1
        bad[1] = 0                                              # ... also when there is nothing to do
        assert fn(*bad) == -1


def test_the_host_entry_refuses_non_finite_weights():
    fn = api.lib().mir_optimize_least_squares_batched16_ex_d
    for value in (np.nan, np.inf, -np.inf):
        good, keep = _good()
        keep[7][ROWS // 2] = value
        assert fn(*good) == -1, value


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("model", [16, 17])
def test_no_problems_is_answered_without_a_device(entry, model):
    fn = getattr(api.lib(), entry)
    good, keep = _good(n=16 if model == 16 else 11, model=model)
    good[1] = 0
    assert fn(*good) == 0
    good[2] = 5000                                              # ... whatever m is (the weights are then not read: 40 of them)
    ex = api.BatchedExtras(covariance=keep[8].ctypes.data)
    good[12] = C.byref(ex)
    assert fn(*good) == 0
    if entry in FIT_ENTRIES:                                    # no extras: the fit entries are then the old ones
        good[12] = None
        assert fn(*good) == 0


def test_python_wrapper_checks_and_routes(monkeypatch):
    L = api.lib()
    old, new = [], []

    def spy_old(*a):
        old.append(a)
        return 0

    def spy_new(*a):
        new.append(a)
        return 0
    monkeypatch.setattr(L, "mir_optimize_least_squares_batched16_d", spy_old)
    monkeypatch.setattr(L, "mir_optimize_least_squares_batched16_ex_d", spy_new)
    x = np.ones((2, 16)); t = np.linspace(0, 4, 40); d = np.zeros((2, 40))
    fit = M.optimizeLeastSquaresBatched16
    for bad in (dict(x=x.astype(np.float32)), dict(t=t.astype(np.float32)), dict(data=d.astype(np.float32)),
                dict(weights=np.ones(40, np.float32))):
        a = dict(x=x, t=t, data=d); a.update(bad)
        with pytest.raises(ValueError, match="float64"):
            fit(M.MODEL16_EXP_HARM16, a.pop("x"), a.pop("t"), a.pop("data"), **a)
    for model in (M.MODEL_EXP_DECAY, M.MODEL_EXP_DECAY_PAD8, 18):
        with pytest.raises(ValueError):
            fit(model, x, t, d, weights=np.ones(40))
    for w in (np.ones(39), np.ones((2, 39)), np.ones((3, 40)), np.ones((40, 2)), np.ones((1, 2, 40))):
        with pytest.raises(ValueError, match="weights"):
            fit(M.MODEL16_EXP_HARM16, x, t, d, weights=w)
    with pytest.raises(ValueError):
        fit(M.MODEL16_EXP_HARM16, x, np.linspace(0, 4, 41), d, covariance=True)
    with pytest.raises(ValueError):
        fit(M.MODEL16_EXP_HARM16, x, t, np.zeros((3, 40)), covariance=True)
    with pytest.raises(ValueError):
        fit(M.MODEL16_EXP_HARM16, x, t, d, l=np.zeros(15), covariance=True)
    assert not old and not new
    # no extras: the call optimizeLeastSquaresBatched makes
    res, xo = fit(M.MODEL16_EXP_HARM16, x, t, d)
    assert len(old) == 1 and not new and old[0][3] == 16 and old[0][1] == 2 and old[0][2] == 40 and old[0][12] is None
    assert xo.dtype == np.float64 and len(res) == 2
    # with extras: the new entry, with the struct filled in
    out = fit(M.MODEL16_EXP_HARM16, x, t, d, weights=np.ones((2, 40)), covariance=True, absolute_sigma=True, variant=2)
    assert len(out) == 3 and out[2].shape == (2, 16, 16) and len(old) == 1 and len(new) == 1
    ex = new[0][12]._obj
    assert ex.struct_size == C.sizeof(api.BatchedExtras) and ex.flags == 1 and ex.weights and ex.weight_stride == 40 and ex.covariance
    assert new[0][11]._obj.variant == 2
    out = fit(M.MODEL16_GAUSS3_AFFINE, np.ones((2, 11)), t, d, weights=np.ones(40))
    assert len(out) == 2 and len(new) == 2 and new[1][12]._obj.weight_stride == 0 and not new[1][12]._obj.covariance
    out = fit(M.MODEL16_EXP_HARM16, x, t, d, covariance=True)
    assert len(out) == 3 and len(new) == 3 and not new[2][12]._obj.weights and new[2][12]._obj.flags == 0
    # the old route still refuses, and says where to go
    with pytest.raises(ValueError, match="optimizeLeastSquaresBatched16"):
        M.optimizeLeastSquaresBatched(M.MODEL16_EXP_HARM16, x, t, d, dtype=np.float64, covariance=True)


def test_weighted_n16_user_models_build_against_the_public_header_and_export_their_entries():
    path = hipbuild.user_model_n16_weighted_lib()      # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    L = C.CDLL(path)
    for n in (9, 13):
        assert getattr(L, f"user_fit_weighted_harm{n}_d") and getattr(L, f"user_weighted_harm{n}_covariance_d")
    blob = open(path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"k_lm_batched16" in blob and b"k_batched16_covariance" in blob and b"HarmILi9" in blob and b"HarmILi13" in blob


@pytest.mark.parametrize("key", WP16.SETS, ids=lambda k: f"{k[0]}-n{k[1]}-m{k[2]}")
def test_the_sets_are_fit_for_the_gpu_test(oracle, key):
    ref = WP16.oracle_fits(oracle, key)
    unweighted = WP16.oracle_fits(oracle, key, weighted=False)
    again = WP16.oracle_fits(oracle, key, reverse=True)
    count = len(ref)
    assert count == WP16.COUNT and all(r.status >= 0 for r, _ in ref), [int(r.status) for r, _ in ref]
    w = WP16.model_of(key)[3]
    zeros = np.count_nonzero(w == 0, axis=1)
    expected = WP16.ZERO_TAIL if key[2] - WP16.ZERO_TAIL >= 4 * key[1] else 0
    assert (zeros[0::4] == expected).all() and not zeros[np.arange(count) % 4 != 0].any()
    dist = [float(np.max(np.abs(xu - x) / np.abs(x))) for (_, x), (_, xu) in zip(ref, unweighted)]
    for k, ((_, x), (_, xu)) in enumerate(zip(ref, unweighted)):
        assert not np.allclose(xu, x, rtol=1e-6, atol=0.0), (k, x, xu)
    tight = sum(1 for (r, x), (r2, x2) in zip(ref, again) if r2.status >= 0 and gaps(r2, x2, r, x)[0])
    cond, gap = WP16.reference_figures(key, np.array([x for _, x in ref]))
    dof = [np.count_nonzero(wk) - key[1] for wk in w[0::4]]
    wrong = max((key[2] - key[1]) / d - 1 for d in dof)
    print(f"{key}: weighted against unweighted minimiser, smallest relative distance {min(dist):.2e}; rows reversed: {tight} of "
          f"{count} tight; cond of the equilibrated J^T J <= {cond:.2e}; covariance gap, central differences at 2^-26 against "
          f"the analytic J: {gap:.2e} (recorded {WP16.CPU_FD_GAP[key]:.1e}, GPU bar {WP16.fd_bar(key):.0e}; analytic GPU bar "
          f"{100 * 2.0 ** -52 * cond:.1e}); a dof of m - n would move it by {wrong:.1e}")
    assert tight >= 0.95 * count, tight
    assert WP16.CPU_FD_GAP[key] / 2 <= gap <= 2 * WP16.CPU_FD_GAP[key], (gap, WP16.CPU_FD_GAP[key])
