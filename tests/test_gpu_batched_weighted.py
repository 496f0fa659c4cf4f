"""Per-row weights and parameter covariance on the batched one-wavefront-per-problem path, on the GPU, in both precisions.

Problem sets: tests/weighted_problems.py (heteroscedastic data, w = 1 / sigma, every fourth problem with 37 zero weights).
Fits are compared with the oracle minimising the WEIGHTED objective (a Python f returning w (model - d)):
  f64  at the bar of tests/test_gpu_batched_f64.py (its `agree`: status class on every problem, residual rtol 1e-9 and x
       rtol 1e-6 on at least 95 % of the problems, the rest within 1e-7 / 1e-3);
  fp32 against the float oracle at the bar of test_cfg5_pad8_all_4096_problems_match_the_float_oracle (tests/test_gpu_batched.py):
       residual rtol 1e-3; err = max_j |x - x_o| / max(1, |x_o|): median <= 1e-4, 99 % quantile <= 5e-3, max <= 5e-2.
The unweighted minimiser of these problems differs from the weighted one beyond rtol 1e-6 on all of them
(tests/test_batched_weighted_host.py), so a fit that ignored its weights fails here.

Covariance: the reference is numpy float64, the analytic model Jacobian at the returned x, inv(J^T J) residual / dof, compared
entry-wise scaled by sd_i sd_j (weighted_problems.scaled_gap). What the reference side gives on its own on the 64 EXP_DECAY
problems: cond(J^T J) <= 1.0e3; float64 central differences at h = 2^-26 against the analytic Jacobian move the measure by at
most 4.9e-9, rounding J to float alone by 2.9e-8. The bars are 10 x the larger of the device's measured worst gap and (for
f64) the CPU's 4.9e-9, rounded up to one digit -- the margin covers the device's exp and its summation order:
                       measured worst gap (MI355X)                                   bar
  f64 analytic (user model, grad)      2.8e-14   (below the CPU's 4.9e-9)             5e-8
  f64 FD  EXP_DECAY                    6.3e-9    (weighted 5.2e-9, unweighted 6.3e-9) 7e-8
  f64 FD  user model                   7.6e-9                                         8e-8
  f64 FD  EXP_DECAY_PAD8               1.2e-7    (weighted 8.1e-8, unweighted 1.2e-7) 2e-6
  f32 analytic (user model, grad)      7.5e-6                                         8e-5
  f32 FD  EXP_DECAY                    1.3e-4    (weighted 1.1e-4, unweighted 1.3e-4) 2e-3
  f32 FD  user model                   1.6e-4                                         2e-3
  f32 FD  EXP_DECAY_PAD8               3.2e-2    (weighted 1.7e-2, unweighted 3.2e-2) 4e-1
(one bar per model family rather than the loosest for all: the eight-parameter family amplifies a Jacobian error about 20
times more in double and 250 times more in float than the three-parameter one. A wrong count of the degrees of freedom --
m - n for a problem with 37 zero weights -- moves the measure by 7.8e-2: outside every bar but the last.)
(profiles/r08/batched_weighted.txt holds the same figures). Every comparison prints its worst gap before it asserts.
"""
import ctypes as C

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import problems as P
import test_gpu_batched_f64 as F64
import weighted_problems as WP

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
ANALYTIC = 2                                        # MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN
# the covariance bars: see the module docstring
COV_BAR = {(np.float64, "analytic", "user"): 5e-8, (np.float64, "fd", M.MODEL_EXP_DECAY): 7e-8, (np.float64, "fd", "user"): 8e-8,
           (np.float64, "fd", M.MODEL_EXP_DECAY_PAD8): 2e-6, (np.float32, "analytic", "user"): 8e-5,
           (np.float32, "fd", M.MODEL_EXP_DECAY): 2e-3, (np.float32, "fd", "user"): 2e-3, (np.float32, "fd", M.MODEL_EXP_DECAY_PAD8): 4e-1}


def rdt(dtype):
    f = "<f4" if dtype == np.float32 else "<f8"
    return np.dtype([("status", "<i4"), ("iterations", "<u4"), ("fCalls", "<u4"), ("gCalls", "<u4"), ("residual", f), ("lambda", f)])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def records(res, dtype):
    return [(int(r.status), r.iterations, r.fCalls, r.gCalls, dtype(r.residual).tobytes(), dtype(r.lambda_).tobytes()) for r in res]


def cast(dtype, *arrays):
    return [None if a is None else np.ascontiguousarray(a, dtype=dtype) for a in arrays]


def launch_device(fn, dtype, n, x0, t, data, w=None, lo=None, up=None, variant=0, flags=0, cov=True, reps=1, model=None,
                  cov_fn=None):
    """An _ex launch on device data: fn is mir_lsq_batched_kernel_ex_* (with `model`) or a user library's entry (without).
    Returns per launch (records, x, cov). With cov_fn (a covariance-only entry), its result on the LAST launch's device data
    is appended to the list."""
    count, m = data.shape
    x0, t, data, w = cast(dtype, x0, t, data, w)
    lo = np.full(n, -np.inf, dtype) if lo is None else np.asarray(lo, dtype)
    up = np.full(n, np.inf, dtype) if up is None else np.asarray(up, dtype)
    s = M.LeastSquaresSettings(dtype)
    item = np.dtype(dtype).itemsize
    R = rdt(dtype)
    bufs = [api.DeviceBuffer(a) for a in (t, data, x0, lo, up)]
    dt_, dd, dx, dlo, dup = bufs
    dres = api.DeviceBuffer(nbytes=count * R.itemsize, dtype=np.uint8, shape=(count * R.itemsize,))
    rows = (count if t.ndim == 2 else 1) * m
    dbasis = api.DeviceBuffer(nbytes=rows * 4 * item, dtype=dtype, shape=(rows, 4))
    dcov = api.DeviceBuffer(nbytes=count * n * n * item, dtype=dtype, shape=(count, n, n))
    dw = api.DeviceBuffer(w) if w is not None else None
    st = api.Stream()
    opt = api.BatchedOptions(stream=st.handle, basis=dbasis.ptr, basis_bytes=rows * 4 * item, variant=variant)
    ex = api.BatchedExtras(flags=flags, weights=dw.ptr if dw else None, weight_stride=0 if (w is None or w.ndim == 1) else m,
                           covariance=dcov.ptr if cov else None)
    t_stride = 0 if t.ndim == 1 else m
    head = [C.byref(s), count, m] + ([model] if model is not None else [])
    outs = []
    for _ in range(reps):
        dx.upload(x0)
        dcov.upload(np.full((count, n, n), 7.0, dtype))
        rc = fn(*head, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr, dres.ptr, C.byref(opt), C.byref(ex))
        assert rc == 0, rc
        st.synchronize()
        outs.append((np.frombuffer(dres.download().tobytes(), dtype=R).copy(), dx.download().reshape(count, n).copy(),
                     dcov.download().copy() if cov else None))
    if cov_fn is not None:
        dcov.upload(np.full((count, n, n), 7.0, dtype))
        rc = cov_fn(*head, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr, dres.ptr, C.byref(opt), C.byref(ex))
        assert rc == 0, rc
        st.synchronize()
        outs.append(dcov.download().copy())
    for b in bufs + [dres, dbasis, dcov] + ([dw] if dw else []):
        b.free()
    return outs


def kernel_ex(dtype):
    return getattr(api.lib(), "mir_lsq_batched_kernel_ex_" + ("s" if dtype == np.float32 else "d"))


def covariance_entry(dtype):
    return getattr(api.lib(), "mir_lsq_batched_covariance_" + ("s" if dtype == np.float32 else "d"))


def check_fits(dtype, status, resid, x, ref, label):
    """the parity bar of the module docstring. ref: per problem (oracle result, oracle x)"""
    count = len(ref)
    if dtype == np.float64:
        loose = []
        for k, (ro, xo) in enumerate(ref):
            r = type("R", (), {"status": status[k], "residual": resid[k]})
            F64.agree(k, r, x[k], ro, xo, loose)
        print(f"{label} f64: {len(loose)} of {count} outside the tight bar: {loose}")
        assert len(loose) <= 0.05 * count, loose
        return
    ro_st = np.array([int(ro.status) for ro, _ in ref]); ro_res = np.array([ro.residual for ro, _ in ref])
    xo = np.array([xk for _, xk in ref], dtype=np.float64)
    assert np.all((np.asarray(status) >= 0) == (ro_st >= 0)), (status, ro_st)
    ok = ro_st >= 0
    rgap = np.abs(np.asarray(resid, dtype=np.float64)[ok] / ro_res[ok] - 1)
    err = (np.abs(x.astype(np.float64) - xo) / np.maximum(1.0, np.abs(xo))).max(axis=1)[ok]
    print(f"{label} f32: residual gap max {rgap.max():.3e}; x err median {np.median(err):.3e} q99 {np.quantile(err, 0.99):.3e} "
          f"max {err.max():.3e}")
    assert rgap.max() <= 1e-3, rgap.max()
    assert np.median(err) <= 1e-4 and np.quantile(err, 0.99) <= 5e-3 and err.max() <= 5e-2, (np.median(err), err.max())


def oracle_refs(oracle, dtype, model, t, data, x0, w, lower=None):
    out = []
    for k in range(data.shape[0]):
        f = WP.weighted_f(model, t, data[k], w if w.ndim == 1 else w[k], dtype=dtype)
        out.append(oracle.optimize(f, t.size, np.asarray(x0[k], dtype=dtype), lower=lower, dtype=dtype))
    return out


def covariance_gaps(jac, t, data, w, x, cov, absolute_sigma=False, value=None):
    """worst scaled gap of `cov` against the numpy float64 reference at the returned x; jac(t, p) the analytic m x n Jacobian,
    value(t, p) the model (for the float64 residual at x)"""
    worst = 0.0
    for k in range(x.shape[0]):
        wk = np.asarray(w if np.ndim(w) == 1 else w[k], dtype=np.float64)
        xk = x[k].astype(np.float64)
        r = wk * (value(np.asarray(t, np.float64), xk) - np.asarray(data[k], np.float64))
        ref = WP.reference_covariance(jac(t, xk), wk, r @ r, absolute_sigma)
        assert np.all(np.isfinite(cov[k])), (k, cov[k])
        assert (bits(cov[k]) == bits(cov[k].T.copy())).all(), k              # symmetric, bit for bit
        worst = max(worst, WP.scaled_gap(cov[k], ref))
    return worst


def builtin(model):
    return (lambda t, p: WP.model_jacobian(model, t, p)), (lambda t, p: WP.model_value(model, t, p))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", [M.MODEL_EXP_DECAY, M.MODEL_EXP_DECAY_PAD8])
def test_weights_of_ones_give_the_bits_of_the_unweighted_fit(model, dtype):
    """... which ties the weighted instance to the fused float oracle through the bit-exact tests of tests/test_gpu_batched.py"""
    count = 128
    t, data, x0, w = WP.MAKERS[model](count)
    res0, xa = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype)
    res1, xb = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, weights=np.ones_like(w))
    res2, xc = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, weights=np.ones(t.size))
    assert (bits(xa) == bits(xb)).all() and (bits(xa) == bits(xc)).all()
    assert records(res0, dtype) == records(res1, dtype) == records(res2, dtype)
    assert sum(r.iterations for r in res0) > 3 * count and all(r.status >= 0 for r in res0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", [M.MODEL_EXP_DECAY, M.MODEL_EXP_DECAY_PAD8])
def test_weighted_fits_match_the_oracle_on_the_weighted_objective(oracle, model, dtype):
    count = 64
    t, data, x0, w = WP.MAKERS[model](count)
    t, data, x0, w = cast(dtype, t, data, x0, w)
    res, x = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, weights=w)
    ref = oracle_refs(oracle, dtype, model, t, data, x0, w)
    if dtype == np.float64:
        assert all(ro.status >= 0 for ro, _ in ref)
    check_fits(dtype, [int(r.status) for r in res], [r.residual for r in res], x, ref, f"weighted model {model}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", [M.MODEL_EXP_DECAY, M.MODEL_EXP_DECAY_PAD8])
def test_zero_weights_equal_shorter_problems(model, dtype):
    """Rows of weight 0, filled with garbage data, against the truncated problems launched on their own with a smaller m. Every
    zero-weight row contributes exact zeros to every sum, so the two fits are expected to agree bit for bit (printed); the
    assertion is the parity bar."""
    count, m = 64, 512
    t, data, x0, w = WP.MAKERS[model](4 * count, m)
    sel = slice(0, 4 * count, 4)                                         # the problems with 37 zero weights
    t, data, x0, w = cast(dtype, t, data[sel], x0[sel], w[sel])
    assert (w[:, m - WP.ZERO_TAIL:] == 0).all() and (w[:, :m - WP.ZERO_TAIL] != 0).all()
    garbage = data.copy()
    u = P.splitmix64_uniform(4242, count * WP.ZERO_TAIL).reshape(count, WP.ZERO_TAIL)
    garbage[:, m - WP.ZERO_TAIL:] = 1e3 * (u - 0.5)
    res_a, xa = M.optimizeLeastSquaresBatched(model, x0, t, garbage, dtype=dtype, weights=w)
    ms = m - WP.ZERO_TAIL
    res_b, xb = M.optimizeLeastSquaresBatched(model, x0, t[:ms], data[:, :ms], dtype=dtype, weights=w[:, :ms])
    same = (bits(xa) == bits(xb)).all() and records(res_a, dtype) == records(res_b, dtype)
    print(f"zero weights against truncation, model {model} {np.dtype(dtype).name}: bit-identical = {same}")
    ref = [(r, xk.astype(np.float64)) for r, xk in zip(res_b, xb)]
    check_fits(dtype, [int(r.status) for r in res_a], [r.residual for r in res_a], xa, ref, "zero weights")
    assert all(r.status >= 0 for r in res_a)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", [M.MODEL_EXP_DECAY, M.MODEL_EXP_DECAY_PAD8])
def test_shared_weights_give_the_bits_of_tiled_ones(model, dtype):
    count = 64
    t, data, x0, w = WP.MAKERS[model](count)
    res0, xa, ca = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, weights=w[0], covariance=True)
    res1, xb, cb = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, weights=np.tile(w[0], (count, 1)), covariance=True)
    assert (bits(xa) == bits(xb)).all() and records(res0, dtype) == records(res1, dtype) and (bits(ca) == bits(cb)).all()
    w2 = np.tile(w[0], (count, 1)); w2[7] *= 1.5                          # problem 7 sees other weights
    res2, xc = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, weights=w2)
    same = (bits(xa) == bits(xc)).all(axis=1)
    assert same[np.arange(count) != 7].all() and not same[7]


@pytest.mark.parametrize("dtype", DTYPES)
def test_bounded_and_weighted(oracle, dtype):
    """bounded_problems() of tests/test_gpu_batched_f64.py with weights 1 / sigma, sigma from the data by the recipe of the weighted
    sets: the kernel entry answers -100 for the problems whose minimiser is cut off (and NaN for their covariance), the host
    entry completes them with the general solver on the WEIGHTED objective and gives every problem a finite covariance.
    fp32 bar: the one of test_batched_bounded_problems_fall_back_to_general_solver (x rtol 5e-3 atol 5e-4, residual rtol 5e-3)."""
    t, data, x0, lo = F64.bounded_problems()
    count = x0.shape[0]
    w = 1.0 / (0.01 * np.sqrt(np.abs(data) / np.abs(data).max(axis=1, keepdims=True)) + 0.002)
    t, data, x0, w, lo = cast(dtype, t, data, x0, w, lo)
    (raw, _, cov_k), = launch_device(kernel_ex(dtype), dtype, 3, x0, t, data, w, lo=lo, model=M.MODEL_EXP_DECAY)
    needs = set(np.flatnonzero(raw["status"] == -100).tolist())
    assert needs == set(range(0, count, 2)), sorted(needs)
    assert np.isnan(cov_k[0::2]).all() and np.isfinite(cov_k[1::2]).all()
    res, x, cov = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x0, t, data, l=lo, dtype=dtype, weights=w, covariance=True)
    assert all(r.status >= 0 for r in res) and np.all(x[:, 1] >= 1.5) and np.all(x[0::2, 1] == 1.5)
    assert np.isfinite(cov).all() and (bits(cov[1::2]) == bits(cov_k[1::2])).all()
    ref = oracle_refs(oracle, dtype, M.MODEL_EXP_DECAY, t, data, x0, w, lower=lo)
    if dtype == np.float64:
        check_fits(dtype, [int(r.status) for r in res], [r.residual for r in res], x, ref, "bounded")
    else:
        for k, (ro, xo) in enumerate(ref):
            assert ro.status >= 0
            assert np.allclose(x[k], xo, rtol=5e-3, atol=5e-4) and np.isclose(res[k].residual, ro.residual, rtol=5e-3), (k, x[k], xo)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", [M.MODEL_EXP_DECAY, M.MODEL_EXP_DECAY_PAD8])
def test_covariance_with_finite_differences(model, dtype):
    """the built-in models have no grad: central differences at the settings' jacobianEpsilon. With and without
    ABSOLUTE_SIGMA; the problems with 37 zero weights use dof = m - 37 - n (the reference counts the nonzero weights)."""
    count = 64
    t, data, x0, w = WP.MAKERS[model](count)
    t, data, x0, w = cast(dtype, t, data, x0, w)
    jac, value = builtin(model)
    res, x, cov = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, weights=w, covariance=True)
    assert all(r.status >= 0 for r in res)
    gap = covariance_gaps(jac, t, data, w, x, cov, value=value)
    res, xa, cova = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, weights=w, covariance=True, absolute_sigma=True)
    assert (bits(xa) == bits(x)).all()
    gap_abs = covariance_gaps(jac, t, data, w, xa, cova, absolute_sigma=True, value=value)
    # unweighted: dof = m - n
    res, xu, covu = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=dtype, covariance=True)
    gap_u = covariance_gaps(jac, t, data, np.ones(t.size), xu, covu, value=value)
    # the wrong dof (m - n for a problem with 37 zero weights) would move the measure by (m - n) / (m - 37 - n) - 1 = 7.8e-2
    print(f"covariance FD model {model} {np.dtype(dtype).name}: worst scaled gap {gap:.3e}, absolute sigma {gap_abs:.3e}, "
          f"unweighted {gap_u:.3e}")
    bar = COV_BAR[(dtype, "fd", model)]
    assert gap <= bar and gap_abs <= bar and gap_u <= bar, (gap, gap_abs, gap_u, bar)


def peak_value(t, x):
    z = (t - x[1]) / x[2]
    return x[0] * np.exp(-0.5 * z * z) + x[3] + x[4] * t


def peak_jacobian(t, x):
    t = np.asarray(t, np.float64); x = np.asarray(x, np.float64)
    z = (t - x[1]) / x[2]; e = np.exp(-0.5 * z * z)
    return np.stack([e, x[0] * e * z / x[2], x[0] * e * z * z / x[2], np.ones_like(t), t], axis=1)


def make_peaks(count, m=384):
    """tests/user_model/user_model_weighted.hip: a peak on a sloping baseline with noise that grows as the square root of the
    signal, sigma = 0.01 sqrt(clean), w = 1 / sigma (cond(J^T J) <= 7e2 over the set); every fourth problem has 37 masked
    channels (weight 0) in the MIDDLE of the trace"""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 5)); w = np.empty((count, m))
    for k in range(count):
        u = P.splitmix64_uniform(1300 + k, m + 16)
        p = np.array([2.0 + 2.0 * u[0], 1.5 + u[1], 0.4 + 0.3 * u[2], 1.0 + u[3], 0.2 * u[4]])
        clean = peak_value(t, p)
        sigma = 0.01 * np.sqrt(clean)
        data[k] = clean + 1.7 * sigma * (2 * u[16:] - 1)
        w[k] = 1.0 / sigma
        x0[k] = p * (1 + 0.05 * (2 * u[8:13] - 1))
        if k % 4 == 0:
            w[k, 100:100 + WP.ZERO_TAIL] = 0.0
    return t, data, x0, w


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_weighted_user_model(oracle, dtype):
    """tests/user_model/user_model_weighted.hip through the public header only: the weighted fit with the model's own grad and
    with finite differences against the oracle (given the weighted f, and the weighted analytic g where the device uses grad),
    and both covariances against numpy; the covariance-only launcher reproduces the fit launch's covariance bit for bit."""
    count, n = 64, 5
    suf = "s" if dtype == np.float32 else "d"
    UL = C.CDLL(hipbuild.user_model_weighted_lib())
    fit, covfn = getattr(UL, "user_fit_weighted_peak_" + suf), getattr(UL, "user_weighted_peak_covariance_" + suf)
    for fn in (fit, covfn):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 4
    t, data, x0, w = cast(dtype, *make_peaks(count))
    for variant, name in ((ANALYTIC, "analytic"), (0, "fd")):
        (raw, x, cov), cov2 = launch_device(fit, dtype, n, x0, t, data, w, variant=variant, cov_fn=covfn)
        assert (raw["status"] >= 0).all() and ((raw["gCalls"] >= 1) == (variant == ANALYTIC)).all()
        assert (bits(cov) == bits(cov2)).all()
        ref = []
        for k in range(count):
            def f(p, y, k=k):
                y[:] = w[k] * (peak_value(t, np.asarray(p, dtype=dtype)) - data[k])

            def g(p, J, k=k):
                J[:, :] = (w[k].astype(np.float64)[:, None] * peak_jacobian(t, p)).astype(dtype)
            ref.append(oracle.optimize(f, t.size, x0[k], g=g if variant else None, dtype=dtype))
        check_fits(dtype, raw["status"], raw["residual"], x, ref, f"user model {name}")
        gap = covariance_gaps(peak_jacobian, t, data, w, x, cov, value=peak_value)
        print(f"covariance user model {name} {np.dtype(dtype).name}: worst scaled gap {gap:.3e}")
        assert gap <= COV_BAR[(dtype, name, "user")], (gap, COV_BAR[(dtype, name, "user")])


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_covariance(dtype):
    """+inf: (a) no degrees of freedom -- EXP_DECAY with all but three weights 0, through the whole fit; (b) a J^T J that is
    singular EXACTLY -- EXP3_AFFINE at an x whose first amplitude is 0, so that the column of its rate is zero in every row
    (the covariance entry on hand-made records; a J^T J that is singular only up to rounding, as three exponentials fitted to
    one would give, may or may not keep a positive last minor, which is no test). NaN: a badGuess problem, and every problem
    the kernel entry left at -100 (test_bounded_and_weighted). The covariance entry on the device results of a launch
    reproduces that launch's covariance bit for bit."""
    count = 16
    t, data, x0, w = cast(dtype, *WP.exp_decay_weighted(count))
    w3 = np.zeros_like(w); w3[:, [5, 200, 400]] = w[:, [5, 200, 400]]
    w3[1::2] = w[1::2]                                                    # odd problems keep all their rows
    xn = x0.copy(); xn[3, 0] = np.nan
    res, x, cov = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, xn, t, data, dtype=dtype, weights=w3, covariance=True)
    assert int(res[3].status) == -31 and np.isnan(cov[3]).all()
    for k in range(count):
        if k == 3:
            continue
        assert res[k].status >= 0, (k, res[k])
        if k % 2 == 0:
            assert (cov[k] == np.inf).all(), (k, cov[k])
        else:
            assert np.isfinite(cov[k]).all() and (np.diag(cov[k]) > 0).all(), (k, cov[k])
    # (b) and the bit-for-bit reproduction
    t8, d8, x8, w8 = cast(dtype, *WP.pad8_weighted(count))
    (raw, x, cov), cov2 = launch_device(kernel_ex(dtype), dtype, 8, x8, t8, d8, w8, model=M.MODEL_EXP_DECAY_PAD8,
                                        cov_fn=covariance_entry(dtype))
    assert (raw["status"] >= 0).all() and np.isfinite(cov).all() and (bits(cov) == bits(cov2)).all()
    s = M.LeastSquaresSettings(dtype)
    st = api.Stream()
    xs = np.tile(np.array([1.0, 0.5, 0.7, 1.5, 0.4, 5.0, 0.1, 0.05], dtype), (2, 1)); xs[0, 0] = 0.0
    recs = np.zeros(2, dtype=rdt(dtype)); recs["status"] = 1; recs["residual"] = 1.0
    lo = np.full(8, -np.inf, dtype); up = np.full(8, np.inf, dtype)
    bufs = [api.DeviceBuffer(a) for a in (xs, lo, up, t8, d8[:2], recs.view(np.uint8))]
    dcov = api.DeviceBuffer(nbytes=2 * 64 * np.dtype(dtype).itemsize, dtype=dtype, shape=(2, 8, 8))
    ex = api.BatchedExtras(covariance=dcov.ptr)
    rc = covariance_entry(dtype)(C.byref(s), 2, t8.size, M.MODEL_EXP3_AFFINE, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 0,
                                 bufs[4].ptr, bufs[5].ptr, C.byref(api.BatchedOptions(stream=st.handle)), C.byref(ex))
    assert rc == 0
    st.synchronize()
    out = dcov.download()
    for b in bufs + [dcov]:
        b.free()
    assert (out[0] == np.inf).all(), out[0]
    assert not np.isnan(out[1]).any()                                     # a non-negative status never gives NaN


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_identical_weighted_launches_on_device_data_are_bit_identical(dtype):
    count = 256
    t, data, x0, w = WP.pad8_weighted(count)
    (r1, x1, c1), (r2, x2, c2) = launch_device(kernel_ex(dtype), dtype, 8, x0, t, data, w, model=M.MODEL_EXP_DECAY_PAD8, reps=2)
    assert r1.tobytes() == r2.tobytes() and x1.tobytes() == x2.tobytes() and c1.tobytes() == c2.tobytes()
    assert np.all(r1["status"] >= 0) and r1["iterations"].sum() > 3 * count and np.isfinite(c1).all()
