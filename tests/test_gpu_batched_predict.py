"""The fitted curve and its 1-sigma confidence band on the device (k_batched_predict, csrc/batched_predict.h;
mir_lsq_batched_predict_s / _d, mir_lsq_batched16_predict_d, launch_batched_predict<Model> through tests/user_model/
user_model_predict.hip, M.predictBatched), on the GPU.

The kernel takes x and C as inputs, so the cases hand it inputs of their own (tests/predict_cases.py: x the starting points of a
problem set, C the float64 reference covariance at that x, 8 problems, cast to the dtype): the kernel's error is measured apart
from the fit's and the covariance kernel's. Reference: numpy float64 at the rounded inputs. Measures (predict_cases):
    value   |v - v_ref| / max(|v_ref|, 1e-3 max_i |v_ref,i|)
    sigma   |s - s_ref| / sqrt(sum_j g_j^2 C_jj)            the uncancelled magnitude (the band cancels up to 120-fold on PAD8)
Bars: per (precision, Jacobian kind, model family) 10 x the larger of the device's measured worst gap (MI355X, every q of the
cases) and what a numpy restatement of the same arithmetic in the working precision gives (predict_cases.CPU_FIGURE), rounded up
to one digit -- the rule of tests/test_gpu_batched_weighted.py; the margin covers the device's exp / sin and its summation order.
The measured figure is the worst over EVERY comparison of this file that uses the bar (every q, the per-problem box with its
one-sided difference, the end-to-end case at the fitted x): scripts/batched_predict.py gaps.
  family      precision  kind       CPU figure   measured (MI355X)   bar
  EXP_DECAY   f32        value      1.8e-07      2.42e-07            3e-06
  EXP_DECAY   f32        fd         3.3e-04      3.77e-04            4e-03
  EXP_DECAY   f64        value      < 1e-15      2.52e-16            1e-14
  EXP_DECAY   f64        fd         2.0e-08      2.29e-08            3e-07
  EXP3_AFFINE f32        value      2.7e-07      3.18e-07            4e-06
  EXP3_AFFINE f32        fd         1.4e-03      2.28e-03            3e-02
  EXP3_AFFINE f64        value      < 1e-15      6.44e-16            1e-14
  EXP3_AFFINE f64        fd         7.6e-08      8.41e-08            9e-07
  PAD8        f32        value      1.1e-05      7.87e-05            8e-04
  PAD8        f32        fd         4.6e-04      4.02e-04            5e-03
  PAD8        f64        value      < 1e-15      2.52e-14            3e-13
  PAD8        f64        fd         2.7e-08      2.26e-08            3e-07
  EXP_HARM16  f64        value      < 1e-15      5.05e-14            6e-13
  EXP_HARM16  f64        fd         1.2e-07      7.49e-08            2e-06
  EXP_HARM16  f64        analytic   9.7e-15      9.67e-15            1e-13
  GAUSS3      f64        value      < 1e-15      5.70e-16            1e-14
  GAUSS3      f64        fd         1.1e-08      8.24e-09            2e-07
  peak (user) f32        value      1.5e-07      1.38e-07            2e-06
  peak (user) f32        fd         3.3e-04      3.06e-04            4e-03
  peak (user) f32        analytic   1.1e-07      1.31e-07            2e-06
  peak (user) f64        value      < 1e-15      2.56e-16            1e-14
  peak (user) f64        fd         2.1e-08      4.24e-08            5e-07
  peak (user) f64        analytic   < 1e-15      3.04e-16            1e-14
  Harm<13>    f64        value      < 1e-15      1.91e-14            2e-13
  Harm<13>    f64        fd         8.6e-08      6.22e-08            9e-07
  Harm<13>    f64        analytic   1.4e-15      1.35e-15            2e-14
(the CPU figure of the harmonic family at n = 9, which has no instance here: fd 7.2e-08, analytic 1.1e-15. "< 1e-15" enters the
rule as 1e-15. The f32 value gap of PAD8 moves with the grid, by where a query falls beside a zero of the curve: 9.3e-08,
7.9e-05, 1.3e-05, 2.2e-06, 4.8e-06 at q = 1, 63, 64, 65, 129 and 6.0e-05 end to end; the CPU figure is that of q = 129.)
profiles/r25/batched_predict.txt holds the same figures. Every comparison prints its worst gap before it asserts.
The identities (bit for bit) pin every instance independently of any reference; the end-to-end cases run a fit with covariance
and predict at tq = t from the same device buffers."""
import ctypes as C

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import predict_cases as PC
import weighted_problems as WP
import batched16_weighted_problems as WP16
from test_gpu_batched_weighted import bits, rdt

pytestmark = pytest.mark.gpu

ANALYTIC = 2                                        # MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN
PER_PROBLEM = 2                                     # MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM
F32, F64 = np.float32, np.float64

# the device's measured worst gaps (MI355X; the table of the module docstring): (family, dtype name, kind)
DEVICE_GAP = {
    ("exp3", "float32", "fd"): 2.28e-03, ("exp3", "float32", "value"): 3.18e-07,
    ("exp3", "float64", "fd"): 8.41e-08, ("exp3", "float64", "value"): 6.44e-16,
    ("exp_decay", "float32", "fd"): 3.77e-04, ("exp_decay", "float32", "value"): 2.42e-07,
    ("exp_decay", "float64", "fd"): 2.29e-08, ("exp_decay", "float64", "value"): 2.52e-16,
    ("gauss3", "float64", "fd"): 8.24e-09, ("gauss3", "float64", "value"): 5.70e-16,
    ("harm13", "float64", "analytic"): 1.35e-15, ("harm13", "float64", "fd"): 6.22e-08, ("harm13", "float64", "value"): 1.91e-14,
    ("harm16", "float64", "analytic"): 9.67e-15, ("harm16", "float64", "fd"): 7.49e-08, ("harm16", "float64", "value"): 5.05e-14,
    ("pad8", "float32", "fd"): 4.02e-04, ("pad8", "float32", "value"): 7.87e-05,
    ("pad8", "float64", "fd"): 2.26e-08, ("pad8", "float64", "value"): 2.52e-14,
    ("peak", "float32", "analytic"): 1.31e-07, ("peak", "float32", "fd"): 3.06e-04, ("peak", "float32", "value"): 1.38e-07,
    ("peak", "float64", "analytic"): 3.04e-16, ("peak", "float64", "fd"): 4.24e-08, ("peak", "float64", "value"): 2.56e-16,
}


def bar(fam, dtype, kind):
    return PC.bar(fam, dtype, kind, DEVICE_GAP.get((fam, np.dtype(dtype).name, kind), 0.0))


# ---- the instances: name -> (family of predict_cases, dtype, entry, model id or None for a user library, has grad)
def _user(name):
    fn = getattr(C.CDLL(hipbuild.user_model_predict_lib()), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 5
    return fn


INSTANCES = {
    "exp_decay-f32": ("exp_decay", F32, "mir_lsq_batched_predict_s", M.MODEL_EXP_DECAY, False),
    "exp3-f32": ("exp3", F32, "mir_lsq_batched_predict_s", M.MODEL_EXP3_AFFINE, False),
    "pad8-f32": ("pad8", F32, "mir_lsq_batched_predict_s", M.MODEL_EXP_DECAY_PAD8, False),
    "exp_decay-f64": ("exp_decay", F64, "mir_lsq_batched_predict_d", M.MODEL_EXP_DECAY, False),
    "exp3-f64": ("exp3", F64, "mir_lsq_batched_predict_d", M.MODEL_EXP3_AFFINE, False),
    "pad8-f64": ("pad8", F64, "mir_lsq_batched_predict_d", M.MODEL_EXP_DECAY_PAD8, False),
    "harm16": ("harm16", F64, "mir_lsq_batched16_predict_d", M.MODEL16_EXP_HARM16, True),
    "gauss3": ("gauss3", F64, "mir_lsq_batched16_predict_d", M.MODEL16_GAUSS3_AFFINE, False),
    "peak-f32": ("peak", F32, "user_predict_peak_s", None, True),
    "peak-f64": ("peak", F64, "user_predict_peak_d", None, True),
    "harm13": ("harm13", F64, "user_predict_harm13_d", None, True),
}
BUILTIN8 = [k for k, v in INSTANCES.items() if v[3] is not None and v[3] < 16]


def predict(inst, x, tq, cov=None, lo=None, up=None, variant=0, flags=0, guard=0, eps=None):
    """one launch of the instance's entry on device copies of the arguments. Returns (value, sigma or None) -- with guard (bytes)
    the two outputs as flat arrays WITH their guard bands in front and behind."""
    fam, dtype, entry, model, _ = INSTANCES[inst]
    fn = getattr(api.lib(), entry) if model is not None else _user(entry)
    x = np.ascontiguousarray(x, dtype=dtype); tq = np.ascontiguousarray(tq, dtype=dtype)
    count, q = x.shape[0], tq.shape[-1]
    s = M.LeastSquaresSettings(dtype)
    if eps is not None:
        s.jacobianEpsilon = eps
    ins = [None if a is None else api.DeviceBuffer(np.ascontiguousarray(a, dtype=dtype)) for a in (x, lo, up, tq, cov)]
    ptr = [None if b is None else b.ptr for b in ins]
    item = np.dtype(dtype).itemsize
    g = guard // item
    sentinel = np.full(count * q + 2 * g, -777.25, dtype=dtype)
    outs = [api.DeviceBuffer(sentinel) for _ in range(1 if cov is None else 2)]
    st = api.Stream()
    opt = api.BatchedOptions(stream=st.handle, variant=variant)
    ex = api.BatchedExtras(flags=flags)
    head = [C.byref(s), count, q] + ([model] if model is not None else [])
    rc = fn(*head, ptr[0], ptr[1], ptr[2], ptr[3], 0 if tq.ndim == 1 else q, ptr[4], outs[0].ptr + guard,
            outs[1].ptr + guard if cov is not None else None, C.byref(opt), C.byref(ex) if flags else None)
    assert rc == 0, rc
    st.synchronize()
    res = [b.download().copy() for b in outs]
    for b in ins + outs:
        if b is not None:
            b.free()
    st.close()
    if not guard:
        res = [r.reshape(count, q) for r in res]
    return res[0], (res[1] if cov is not None else None)


def inputs(inst):
    fam = PC.family(INSTANCES[inst][0])
    dtype = INSTANCES[inst][1]
    return fam, dtype, fam.x.astype(dtype), fam.C.astype(dtype)


def check(inst, kind, v, s, ref, label):
    """value and sigma against reference() = (value, sigma, magnitude) at the instance's bars"""
    fam, dtype = INSTANCES[inst][0], INSTANCES[inst][1]
    vr, sr, mag = ref
    vg, sg = PC.value_gap(v, vr), PC.sigma_gap(s, sr, mag)
    vb, sb = bar(fam, dtype, "value"), bar(fam, dtype, kind)
    print(f"PREDICT-GAP {fam} {np.dtype(dtype).name} {label}: value {vg:.3e} (bar {vb:.0e})  sigma {kind} {sg:.3e} (bar {sb:.0e})")
    assert np.isfinite(v).all() and np.isfinite(s).all() and (s >= 0).all()
    assert vg <= vb, (vg, vb)
    assert sg <= sb, (sg, sb)


@pytest.mark.parametrize("q", PC.QS)
@pytest.mark.parametrize("inst", BUILTIN8)
def test_builtin_models_value_and_band_by_central_differences(inst, q):
    fam, dtype, x, cov = inputs(inst)
    tq = PC.grid(q, dtype)
    v, s = predict(inst, x, tq, cov)
    check(inst, "fd", v, s, PC.reference(fam, x, cov, tq), f"q={q}")
    v0, _ = predict(inst, x, tq)                                          # without sigma: the same values
    assert (bits(v0) == bits(v)).all()


@pytest.mark.parametrize("inst,variant", [("harm16", 0), ("harm16", ANALYTIC), ("gauss3", 0)])
def test_wide_builtin_models(inst, variant):
    fam, dtype, x, cov = inputs(inst)
    for q in (65, 129):
        tq = PC.grid(q, dtype)
        v, s = predict(inst, x, tq, cov, variant=variant)
        check(inst, "analytic" if variant else "fd", v, s, PC.reference(fam, x, cov, tq), f"q={q}")


@pytest.mark.parametrize("inst", ["peak-f32", "peak-f64", "harm13"])
def test_the_user_library(inst):
    """tests/user_model/user_model_predict.hip through the public header only: the model's own grad, and central differences"""
    fam, dtype, x, cov = inputs(inst)
    tq = PC.grid(129, dtype)
    ref = PC.reference(fam, x, cov, tq)
    for variant, kind in ((ANALYTIC, "analytic"), (0, "fd")):
        v, s = predict(inst, x, tq, cov, variant=variant)
        check(inst, kind, v, s, ref, "q=129")


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_identities_bit_for_bit(inst):
    fam, dtype, x, cov = inputs(inst)
    n = fam.n
    full = PC.grid(129, dtype)
    out = {q: predict(inst, x, full[:q], cov) for q in (64, 65, 129)}
    v, s = out[129]
    # two launches
    v2, s2 = predict(inst, x, full, cov)
    assert (bits(v) == bits(v2)).all() and (bits(s) == bits(s2)).all()
    # a shared tq against the same tq tiled per problem
    vt, st_ = predict(inst, x, np.tile(full, (PC.COUNT, 1)), cov)
    assert (bits(v) == bits(vt)).all() and (bits(s) == bits(st_)).all()
    # per-problem abscissae are honoured: problem 3 on a grid of its own
    tq2 = np.tile(full, (PC.COUNT, 1)); tq2[3] = tq2[3] + dtype(0.125)
    vs, ss = predict(inst, x, tq2, cov)
    same = (bits(v) == bits(vs)).all(axis=1)
    assert same[np.arange(PC.COUNT) != 3].all() and not same[3]
    # prefixes: 64 of 65, 65 of 129
    for a, b in ((64, 65), (65, 129)):
        assert (bits(out[a][0]) == bits(out[b][0][:, :a])).all() and (bits(out[a][1]) == bits(out[b][1][:, :a])).all()
    # a problem launched alone
    for k in (0, 5):
        vk, sk = predict(inst, x[k:k + 1], full, cov[k:k + 1])
        assert (bits(vk[0]) == bits(v[k])).all() and (bits(sk[0]) == bits(s[k])).all()
    # NULL bounds against infinite ones, shared and per problem
    for shape, flags in (((n,), 0), ((PC.COUNT, n), PER_PROBLEM)):
        vb, sb = predict(inst, x, full, cov, lo=np.full(shape, -np.inf), up=np.full(shape, np.inf), flags=flags)
        assert (bits(v) == bits(vb)).all() and (bits(s) == bits(sb)).all()
    # rows that differ between problems give values that differ
    assert not (bits(v[0]) == bits(v[1])).all() and not (bits(s[0]) == bits(s[1])).all()


@pytest.mark.parametrize("inst", ["exp_decay-f32", "pad8-f32", "pad8-f64", "harm16", "peak-f64"])
def test_fixed_parameters_and_clipped_differences(inst):
    """A box per problem: parameter 1 of problem 3 is fixed, parameter 0 of problem 5 sits on its upper bound (a one-sided
    difference). sigma against the numpy reference with the reduced covariance and the one-sided difference, at the bar of the
    central differences; row and column 1 of problem 3's C are not read."""
    fam, dtype, x, cov = inputs(inst)
    n = fam.n
    tq = PC.grid(129, dtype)
    lo = np.full((PC.COUNT, n), -np.inf, dtype); up = np.full((PC.COUNT, n), np.inf, dtype)
    lo[3, 1] = up[3, 1] = x[3, 1]
    up[5, 0] = x[5, 0]
    v, s = predict(inst, x, tq, cov, lo=lo, up=up, flags=PER_PROBLEM)
    check(inst, "fd", v, s, PC.reference(fam, x, cov, tq, lo, up, eps=PC.EPS[dtype]), "per-problem box")
    v0, s0 = predict(inst, x, tq, cov)
    same = (bits(s) == bits(s0)).all(axis=1)
    assert same[[0, 1, 2, 4, 6, 7]].all() and not same[3] and not same[5] and (bits(v) == bits(v0)).all()
    cov7 = cov.copy(); cov7[3, 1, :] = 7.0; cov7[3, :, 1] = 7.0
    v7, s7 = predict(inst, x, tq, cov7, lo=lo, up=up, flags=PER_PROBLEM)
    assert (bits(v7) == bits(v)).all() and (bits(s7) == bits(s)).all()
    covn = cov.copy(); covn[3, 1, :] = np.nan; covn[3, :, 1] = np.inf
    _, sn = predict(inst, x, tq, covn, lo=lo, up=up, flags=PER_PROBLEM)
    assert (bits(sn) == bits(s)).all()
    if INSTANCES[inst][4]:                                               # the analytic gradient drops the fixed parameter too
        va, sa = predict(inst, x, tq, cov, lo=lo, up=up, flags=PER_PROBLEM, variant=ANALYTIC)
        lo5 = lo.copy(); up5 = up.copy(); up5[5, 0] = np.inf               # (a bound that is not a fixing does not touch grad)
        check(inst, "analytic", va, sa, PC.reference(fam, x, cov, tq, lo5, up5), "per-problem box, grad")


@pytest.mark.parametrize("inst", ["exp_decay-f32", "pad8-f64", "harm16", "peak-f32"])
def test_propagation_of_the_covariance_conventions(inst):
    fam, dtype, x, cov = inputs(inst)
    n = fam.n
    tq = PC.grid(65, dtype)
    v, s = predict(inst, x, tq, cov)
    c = cov.copy(); c[2] = np.inf; c[6] = np.nan
    lo = np.full((PC.COUNT, n), -np.inf, dtype); up = np.full((PC.COUNT, n), np.inf, dtype)
    lo[4] = up[4] = x[4]                                                  # every parameter of problem 4 is fixed
    c[4] = np.nan                                                        # ... so nothing of its C is read
    v1, s1 = predict(inst, x, tq, c, lo=lo, up=up, flags=PER_PROBLEM)
    assert (bits(v1) == bits(v)).all() and np.isfinite(v1).all()          # value: whatever the covariance says
    assert (s1[2] == np.inf).all() and np.isnan(s1[6]).all() and (bits(s1[4]) == bits(np.zeros_like(s1[4]))).all()
    keep = [0, 1, 3, 5, 7]
    assert (bits(s1[keep]) == bits(s[keep])).all()
    # one free diagonal entry decides: +inf in C_11 only
    c = cov.copy(); c[1, 1, 1] = np.inf
    _, s2 = predict(inst, x, tq, c)
    assert (s2[1] == np.inf).all() and (bits(s2[[0, 2]]) == bits(s[[0, 2]])).all()


@pytest.mark.parametrize("inst", ["pad8-f32", "pad8-f64", "harm16", "peak-f64"])
def test_guard_bands_stay_intact(inst):
    fam, dtype, x, cov = inputs(inst)
    guard = 4096
    g = guard // np.dtype(dtype).itemsize
    tq = PC.grid(65, dtype)
    for arrays in ((x[:5], tq, cov[:5]), (x[:5], np.tile(tq, (5, 1)), None)):
        v, s = predict(inst, arrays[0], arrays[1], arrays[2], guard=guard)
        for out in (v, s):
            if out is None:
                continue
            assert (out[:g] == dtype(-777.25)).all() and (out[g + 5 * 65:] == dtype(-777.25)).all()
            assert out.size == 5 * 65 + 2 * g and (out[g:g + 5 * 65] != dtype(-777.25)).all()
    vref, sref = predict(inst, x[:5], tq, cov[:5])
    assert (bits(v[g:g + 325]) == bits(vref.ravel())).all()


@pytest.mark.parametrize("inst", ["pad8-f32", "exp_decay-f64", "harm16"])
def test_python_wrapper(inst):
    fam, dtype, x, cov = inputs(inst)
    model = INSTANCES[inst][3]
    n = fam.n
    tq = PC.grid(65, dtype)
    v, s = predict(inst, x, tq, cov)
    pv, ps = M.predictBatched(model, x, tq, cov, dtype=dtype)
    assert pv.shape == ps.shape == (PC.COUNT, 65) and (bits(pv) == bits(v)).all() and (bits(ps) == bits(s)).all()
    only = M.predictBatched(model, x, np.tile(tq, (PC.COUNT, 1)), dtype=dtype)
    assert (bits(only) == bits(v)).all()
    lo = np.full((PC.COUNT, n), -np.inf); lo[3, 1] = x[3, 1]
    up = np.full((PC.COUNT, n), np.inf); up[3, 1] = x[3, 1]
    _, s3 = M.predictBatched(model, x, tq, cov, l=lo, u=up, dtype=dtype)
    _, s3d = predict(inst, x, tq, cov, lo=lo, up=up, flags=PER_PROBLEM)
    assert (bits(s3) == bits(s3d)).all() and not (bits(s3[3]) == bits(s[3])).all()
    _, s4 = M.predictBatched(model, x, tq, cov, l=np.full(n, -np.inf), dtype=dtype)      # (n,) bounds, one of them None
    assert (bits(s4) == bits(s)).all()


END_TO_END = {
    "pad8-f32": ("mir_lsq_batched_kernel_ex_s", lambda: WP.pad8_weighted(PC.COUNT, 512)),
    "pad8-f64": ("mir_lsq_batched_kernel_ex_d", lambda: WP.pad8_weighted(PC.COUNT, 512)),
    "harm16": ("mir_lsq_batched16_kernel_ex_d", lambda: [a for i, a in enumerate(WP16.harm_weighted(16, 131)) if i != 1]),
}


@pytest.mark.parametrize("inst", list(END_TO_END))
def test_end_to_end_fit_covariance_predict_on_device_buffers(inst):
    """A weighted fit with covariance on device data, then the prediction at tq = t from the SAME device buffers (x, cov, t):
    sum w^2 (value - data)^2 is the record's residual (rtol 1e-9 in f64, 1e-3 in f32, the bars the fits' residuals are held
    to), and sigma is, at the kernel's bar, the numpy quadratic form of the device's own x and cov."""
    famname, dtype, entry, model, _ = INSTANCES[inst]
    fam = PC.family(famname)
    fit_name, maker = END_TO_END[inst]
    t, data, x0, w = [np.ascontiguousarray(a[:PC.COUNT] if a.ndim == 2 else a, dtype=dtype) for a in maker()]
    count, m, n = PC.COUNT, t.size, fam.n
    item = np.dtype(dtype).itemsize
    R = rdt(dtype)
    s = M.LeastSquaresSettings(dtype)
    dt_, dd, dx, dw = [api.DeviceBuffer(a) for a in (t, data, x0, w)]
    dlo, dup = api.DeviceBuffer(np.full(n, -np.inf, dtype)), api.DeviceBuffer(np.full(n, np.inf, dtype))
    dres = api.DeviceBuffer(nbytes=count * R.itemsize, dtype=np.uint8, shape=(count * R.itemsize,))
    dcov = api.DeviceBuffer(np.full((count, n, n), 7.0, dtype))
    dv, ds = [api.DeviceBuffer(np.full((count, m), -777.25, dtype)) for _ in range(2)]
    st = api.Stream()
    opt = api.BatchedOptions(stream=st.handle)
    ex = api.BatchedExtras(weights=dw.ptr, weight_stride=m, covariance=dcov.ptr)
    L = api.lib()
    rc = getattr(L, fit_name)(C.byref(s), count, m, model, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, 0, dd.ptr, dres.ptr, C.byref(opt), C.byref(ex))
    assert rc == 0, rc
    rc = getattr(L, entry)(C.byref(s), count, m, model, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, 0, dcov.ptr, dv.ptr, ds.ptr, C.byref(opt), None)
    assert rc == 0, rc
    st.synchronize()
    raw = np.frombuffer(dres.download().tobytes(), dtype=R)
    x, cov, v, sg = dx.download().reshape(count, n), dcov.download(), dv.download(), ds.download()
    for b in (dt_, dd, dx, dw, dlo, dup, dres, dcov, dv, ds):
        b.free()
    st.close()
    assert (raw["status"] >= 0).all() and np.isfinite(cov).all()
    ssq = np.sum((w.astype(F64) * (v.astype(F64) - data.astype(F64))) ** 2, axis=1)
    rgap = float(np.max(np.abs(ssq / raw["residual"].astype(F64) - 1)))
    print(f"PREDICT-E2E {inst}: residual gap {rgap:.3e}")
    assert rgap <= (1e-3 if dtype == F32 else 1e-9), rgap
    check(inst, "fd", v, sg, PC.reference(fam, x, cov, t), "end to end")
