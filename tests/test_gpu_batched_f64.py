"""The batched one-wavefront-per-problem fit in DOUBLE (mir_optimize_least_squares_batched_d, mir_lsq_batched_kernel_d,
mir_lsq_batched_posvx_d) against the oracle's double instantiation (oracle/, least_squares.d:877-1176), problem by problem,
at the project's f64 parity bar: same status class on every problem, residual to rtol 1e-9 and x to rtol 1e-6 on at least 95 %
of them; the rest (slow decays: a flat valley of p0 exp(-t p1) against the offset p2, where one side may stop a few ulp of the
objective higher) are held to rtol 1e-7 and 1e-3 (`agree`).
Settings are the double defaults on both sides. Iteration and residual-evaluation COUNTS are not compared: they are decided by
rounding noise here, not by the algorithm. The kernel sums J^T J per lane and across the wave and evaluates exp with the device
library, the oracle sums sequentially with numpy's exp; a central difference with h = 2^-26 turns a last-bit difference of a
residual into a relative difference of ~1e-8 in J, and the defaults (absTolerance = eps, relTolerance = 0) run every fit until
its steps ARE rounding noise -- so the two sides take a different number of rejected end-game passes on most problems (measured
on the device: 59 of 64 EXP_DECAY fits; the general solver mir_optimize_least_squares_gpu_d differs from the batched fit the
same way), while their minima agree as stated. The ladder test below pins the kernel's own trajectory bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import problems as P

pytestmark = pytest.mark.gpu

RDT = np.dtype([("status", "<i4"), ("iterations", "<u4"), ("fCalls", "<u4"), ("gCalls", "<u4"), ("residual", "<f8"),
                ("lambda", "<f8")])


def make_exp_decay(count, m=512):
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); truth = np.empty((count, 3)); x0 = np.empty((count, 3))
    for k in range(count):
        u = P.splitmix64_uniform(100 + k, m + 6)                       # per-problem seed = 100 + problem id
        truth[k] = [1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2]]
        data[k] = truth[k, 0] * np.exp(-t * truth[k, 1]) + truth[k, 2] + 0.01 * (2 * u[6:] - 1)
        x0[k] = truth[k] * (1 + 0.3 * (2 * u[3:6] - 1))
    return t, data, truth, x0


def make_exp3(count, m=512):
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); truth = np.empty((count, 8)); x0 = np.empty((count, 8))
    for k in range(count):
        u = P.splitmix64_uniform(100 + k, m + 16)
        truth[k] = [1.0 + u[0], 0.3 + 0.2 * u[1], 0.6 + 0.5 * u[2], 1.5 + 0.5 * u[3], 0.4 + 0.3 * u[4], 5.0 + 2 * u[5], 0.1 * u[6], 0.05 * u[7]]
        p = truth[k]
        data[k] = (p[0] * np.exp(-t * p[1]) + p[2] * np.exp(-t * p[3]) + p[4] * np.exp(-t * p[5]) + p[6] + p[7] * t
                   + 0.002 * (2 * u[16:] - 1))
        x0[k] = truth[k] * (1 + 0.05 * (2 * u[8:16] - 1))
    return t, data, truth, x0


def make_pad8(count, m=512, noise=0.01):
    """tests/problems.py cfg5_pad8 in float64 (same seeds and formulas)"""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); truth = np.empty((count, 8)); x0 = np.empty((count, 8))
    basis = np.stack([np.sin(2 * t), np.cos(2 * t), np.sin(5 * t), np.cos(5 * t), t])
    for k in range(count):
        u = P.splitmix64_uniform(100 + k, m + 16)
        p = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2], 0.6 * u[3] - 0.3, 0.6 * u[4] - 0.3, 0.6 * u[5] - 0.3,
                      0.6 * u[6] - 0.3, 0.1 * u[7] - 0.05])
        truth[k] = p
        data[k] = p[0] * np.exp(-t * p[1]) + p[2] + p[3:] @ basis + noise * (2 * u[16:] - 1)
        x0[k] = p
        x0[k, :2] *= 1 + 0.2 * (2 * u[8:10] - 1)
        x0[k, 2:] += 0.1 * (2 * u[10:16] - 1)
    return t, data, truth, x0


MAKERS = {M.MODEL_EXP_DECAY: make_exp_decay, M.MODEL_EXP3_AFFINE: make_exp3, M.MODEL_EXP_DECAY_PAD8: make_pad8}


def model_value(model, t, p):
    if model == M.MODEL_EXP_DECAY:
        return p[0] * np.exp(-t * p[1]) + p[2]
    if model == M.MODEL_EXP3_AFFINE:
        return p[0] * np.exp(-t * p[1]) + p[2] * np.exp(-t * p[3]) + p[4] * np.exp(-t * p[5]) + p[6] + p[7] * t
    return (p[0] * np.exp(-t * p[1]) + p[2] + p[3] * np.sin(2 * t) + p[4] * np.cos(2 * t) + p[5] * np.sin(5 * t)
            + p[6] * np.cos(5 * t) + p[7] * t)


def oracle_fit(oracle, model, t, d, x0, lower=None, upper=None):
    def f(p, y):
        y[:] = model_value(model, t, p) - d
    return oracle.optimize(f, t.size, x0, lower=lower, upper=upper, dtype=np.float64)


def agree(k, r, x, rr, xr, loose, curve=None):
    """the parity bar of this file for one problem: r, x against the reference result rr, xr. Residual to rtol 1e-9 and x to
    rtol 1e-6 -- or, for a model whose parameters are not identifiable at the data's noise (EXP3_AFFINE: three exponentials),
    the fitted CURVES to 1e-6 of their own scale. A problem outside that bar goes to `loose`, where it is held to a residual
    within rtol 1e-7 and x (or the curve) within 1e-3: an end game on a flat valley that one side leaves a few ulp higher."""
    assert (r.status >= 0) == (rr.status >= 0), (k, r, rr.status)
    if rr.status < 0:
        return
    if curve is None:
        tight = np.allclose(x, xr, rtol=1e-6, atol=1e-7)      # atol: parameters that sit near zero (offset, trig terms)
        near = np.allclose(x, xr, rtol=1e-3, atol=1e-4)
        gap = float(np.max(np.abs(x - xr) / np.maximum(np.abs(xr), 1e-3)))
    else:
        cx, cr = curve(x), curve(xr)
        gap = float(np.max(np.abs(cx - cr)) / np.max(np.abs(cr)))
        tight, near = gap <= 1e-6, gap <= 1e-3
    rgap = abs(r.residual / rr.residual - 1)
    if not (tight and rgap <= 1e-9):
        loose.append((k, gap, rgap))
        assert near and rgap <= 1e-7, (k, gap, rgap, x, xr)


def compare_with_oracle(oracle, model, t, data, x0, res, x, lower=None, upper=None, loose_ok=0.05):
    count = x.shape[0]
    loose = []
    curve = (lambda p: model_value(model, t, p)) if model == M.MODEL_EXP3_AFFINE else None
    for k in range(count):
        ro, xo = oracle_fit(oracle, model, t, data[k], x0[k], lower, upper)
        agree(k, res[k], x[k], ro, xo, loose, curve)
    assert len(loose) <= loose_ok * count, loose
    return loose


@pytest.mark.parametrize("model,count", [(M.MODEL_EXP_DECAY, 64), (M.MODEL_EXP3_AFFINE, 64), (M.MODEL_EXP_DECAY_PAD8, 256)])
def test_builtin_models_match_the_f64_oracle(oracle, model, count):
    t, data, truth, x0 = MAKERS[model](count)
    res, x = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=np.float64)
    assert x.dtype == np.float64 and all(r.iterations >= 1 for r in res)
    compare_with_oracle(oracle, model, t, data, x0, res, x)


@pytest.mark.parametrize("n", [3, 8])
def test_posvx_d_matches_the_f64_oracle_posvx(oracle, n):
    """posvx_rows in double against the oracle's ?posvx('E','L') in double: well-scaled SPD systems to 1e-13 relative, badly
    scaled ones (diagonal spread 1e8: ?laqsy equilibrates on both sides) as accurate as the oracle, and the info of systems whose
    leading minor of order k is not positive."""
    rng = np.random.default_rng(31 + n)
    count = 256
    Pm = np.zeros((count, n, n)); b = rng.standard_normal((count, n))
    for p in range(count):
        G = rng.standard_normal((2 * n, n))
        if p >= count // 2:
            G = G * np.logspace(-2, 2, n)[None, :]
        A = G.T @ G + 1e-3 * np.eye(n)
        if p % 16 == 5:
            k = 1 + (p // 16) % n
            A[k - 1, k - 1] = -abs(A[k - 1, k - 1])
        Pm[p] = A
    x, info = M.batchedPosvx(Pm, b, dtype=np.float64)
    assert x.dtype == np.float64
    worst = 0.0
    scaled = 0
    for p in range(count):
        o = oracle.posvx(Pm[p], b[p], dtype=np.float64)
        oi = 0 if o["info"] == n + 1 else o["info"]
        assert info[p] == oi, (p, info[p], o["info"])
        if oi != 0:
            assert not x[p].any()
            continue
        eq = o["equed"] == "Y"
        scaled += eq
        xr = np.linalg.solve(Pm[p], b[p])
        if p < count // 2:
            worst = max(worst, np.linalg.norm(x[p] - o["x"]) / np.linalg.norm(o["x"]))
        else:
            assert eq or p % 16 == 5, p
            assert np.linalg.norm(x[p] - xr) <= 4 * np.linalg.norm(o["x"] - xr) + 1e-12 * np.linalg.norm(xr), p
    assert worst <= 1e-13, worst
    assert scaled >= count // 3


@pytest.mark.parametrize("model", [M.MODEL_EXP_DECAY_PAD8, M.MODEL_EXP3_AFFINE, M.MODEL_EXP_DECAY])
def test_lambda_ladder_gives_the_bits_of_the_one_by_one_loop(model):
    count = 256
    t, data, truth, x0 = MAKERS[model](count)
    out = []
    for variant in (0, M.BATCHED_NO_LADDER):
        res, x = M.optimizeLeastSquaresBatched(model, x0, t, data, variant=variant, dtype=np.float64)
        out.append((x.view(np.uint64).copy(), [(int(r.status), r.iterations, r.fCalls, np.float64(r.residual).view(np.uint64),
                                               np.float64(r.lambda_).view(np.uint64)) for r in res]))
    assert (out[0][0] == out[1][0]).all()
    assert out[0][1] == out[1][1]
    assert sum(r[1] for r in out[0][1]) > 4 * count


def bounded_problems(count=32, m=512):
    """p1 >= 1.5: even problems have a true rate of 0.8 .. 1.2 (the minimiser is cut off; they start at p1 = 1.7), odd ones
    2.0 .. 2.4 and start within 3 % of it (the bound stays far away)"""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 3))
    for k in range(count):
        u = P.splitmix64_uniform(700 + k, m + 6)
        p = np.array([1.0 + u[0], (0.8 if k % 2 == 0 else 2.0) + 0.4 * u[1], 0.2 * u[2]])
        data[k] = p[0] * np.exp(-t * p[1]) + p[2] + 0.01 * (2 * u[6:] - 1)
        x0[k] = p * (1 + 0.03 * (2 * u[3:6] - 1))
        if k % 2 == 0:
            x0[k, 1] = 1.7
    lo = np.array([-np.inf, 1.5, -np.inf])
    return t, data, x0, lo


def run_kernel_d(model, x0, t, data, lo=None, up=None, variant=0, settings=None, reps=1):
    """mir_lsq_batched_kernel_d on device data (caller-owned basis table); returns [(records, x)] per launch"""
    count, n = x0.shape
    m = data.shape[1]
    L = api.lib()
    s = settings or M.LeastSquaresSettings(np.float64)
    lo = np.full(n, -np.inf) if lo is None else lo
    up = np.full(n, np.inf) if up is None else up
    t_stride = 0 if t.ndim == 1 else m
    dt_, dd, dx = api.DeviceBuffer(t), api.DeviceBuffer(data), api.DeviceBuffer(x0)
    dlo, dup = api.DeviceBuffer(lo), api.DeviceBuffer(up)
    dres = api.DeviceBuffer(nbytes=count * 32, dtype=np.uint8, shape=(count * 32,))
    rows = (count if t_stride else 1) * m
    dbasis = api.DeviceBuffer(nbytes=rows * 4 * 8, dtype=np.float64, shape=(rows, 4))
    st = api.Stream()
    opt = api.BatchedOptions(stream=st.handle, basis=dbasis.ptr, basis_bytes=rows * 32, variant=variant)
    outs = []
    for _ in range(reps):
        dx.upload(x0)
        rc = L.mir_lsq_batched_kernel_d(C.byref(s), count, m, model, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr,
                                        dres.ptr, C.byref(opt))
        assert rc == 0, rc
        st.synchronize()
        outs.append((np.frombuffer(dres.download().tobytes(), dtype=RDT).copy(), dx.download().reshape(count, n).copy()))
    for b in (dt_, dd, dx, dlo, dup, dres, dbasis):
        b.free()
    return outs


def test_bounded_steps_go_to_the_general_solver_and_match_the_bounded_oracle(oracle):
    t, data, x0, lo = bounded_problems()
    count = x0.shape[0]
    (raw, _), = run_kernel_d(M.MODEL_EXP_DECAY, x0, t, data, lo=lo)
    needs = set(np.flatnonzero(raw["status"] == -100).tolist())          # MIR_LSQ_BATCHED_NEEDS_GENERAL
    assert needs == set(range(0, count, 2)), sorted(needs)
    res, x = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x0, t, data, l=lo, dtype=np.float64)
    assert all(r.status >= 0 for r in res) and np.all(x[:, 1] >= 1.5)
    assert np.all(x[0::2, 1] == 1.5)                                     # the bound binds where the minimiser is cut off
    compare_with_oracle(oracle, M.MODEL_EXP_DECAY, t, data, x0, res, x, lower=lo)


@pytest.mark.parametrize("model", [M.MODEL_EXP_DECAY_PAD8, M.MODEL_EXP_DECAY])
def test_per_problem_abscissae_give_the_bits_of_shared_ones(model):
    count = 64
    t, data, truth, x0 = MAKERS[model](count)
    res0, xa = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=np.float64)
    t2 = np.tile(t, (count, 1))
    res1, xb = M.optimizeLeastSquaresBatched(model, x0, t2, data, dtype=np.float64)
    assert (xa.view(np.uint64) == xb.view(np.uint64)).all()
    assert [(int(r.status), r.iterations, r.fCalls) for r in res0] == [(int(r.status), r.iterations, r.fCalls) for r in res1]
    t3 = t2.copy()
    t3[7] *= 1.01                                                       # problem 7 sees other abscissae
    res2, xc = M.optimizeLeastSquaresBatched(model, x0, t3, data, dtype=np.float64)
    same = (xa.view(np.uint64) == xc.view(np.uint64)).all(axis=1)
    assert same[np.arange(count) != 7].all() and not same[7]


def test_validation_codes_match_the_float_entry():
    t, data, truth, x0 = make_exp_decay(4)
    S = M.LeastSquaresStatus
    for field, value in (("minStepQuality", 2.0), ("goodStepQuality", -1.0), ("lambdaIncrease", 0.5), ("lambdaDecrease", 2.0)):
        codes = []
        for dt in (np.float32, np.float64):
            s = M.LeastSquaresSettings(dt)
            setattr(s, field, value)
            res, _ = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x0, t, data, settings=s, dtype=dt)
            codes.append([int(r.status) for r in res])
        assert codes[0] == codes[1] and codes[0][0] < 0, (field, codes)
    s = M.LeastSquaresSettings(np.float64); s.lambdaIncrease = 1e200       # above sqrt(DBL_MAX): LS:941 in double
    res, _ = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x0, t, data, settings=s, dtype=np.float64)
    assert all(r.status == S.badLambdaParams for r in res)
    xn = x0.copy(); xn[1, 0] = np.nan
    res, _ = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, xn, t, data, dtype=np.float64)
    assert res[1].status == S.badGuess and int(res[1].status) == -31 and res[0].status >= 0
    lo = np.array([5.0, -np.inf, -np.inf])
    res, _ = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, x0, t, data, l=lo, dtype=np.float64)
    assert all(int(r.status) == -32 for r in res)
    # (n + 2) m doubles <= 160 KiB - 512: m = 2041 at n = 8 fits, 2042 does not
    tb, db, _, xb = make_pad8(2, 2041)
    res, _ = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY_PAD8, xb, tb, db, dtype=np.float64)
    assert all(r.status >= 0 for r in res)
    tb, db, _, xb = make_pad8(2, 2042)
    with pytest.raises(RuntimeError, match="-3"):
        M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY_PAD8, xb, tb, db, dtype=np.float64)
    s = M.LeastSquaresSettings(np.float64)
    L = api.lib()
    raw = (api._Rd * 1)()
    assert L.mir_lsq_batched_kernel_d(C.byref(s), 0, 2042, M.MODEL_EXP_DECAY_PAD8, xb.ctypes.data, lo.ctypes.data, lo.ctypes.data,
                                      tb.ctypes.data, 0, db.ctypes.data, raw, None) == 0        # count = 0: nothing to launch
    res, x = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY, np.zeros((0, 3)), t, np.zeros((0, t.size)), dtype=np.float64)
    assert res == [] and x.shape == (0, 3)


def test_two_launches_on_device_data_are_bit_identical():
    count = 256
    t, data, truth, x0 = make_pad8(count)
    (r1, x1), (r2, x2) = run_kernel_d(M.MODEL_EXP_DECAY_PAD8, x0, t, data, reps=2)
    assert r1.tobytes() == r2.tobytes() and x1.tobytes() == x2.tobytes()
    assert np.all(r1["status"] >= 0) and r1["iterations"].sum() > 3 * count


def test_batched_fit_agrees_with_the_general_solver_on_the_same_model(oracle):
    """16 PAD8 problems: the batched f64 fit against mir_optimize_least_squares_gpu_d driven by a device callback of the same
    double model (launch_model_residual<ModelExpDecayPad8D>, tests/user_model/user_model_f64.hip), at the bar of this file."""
    count, n = 16, 8
    t, data, truth, x0 = make_pad8(count)
    res, x = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY_PAD8, x0, t, data, dtype=np.float64)
    UL = C.CDLL(hipbuild.user_model_f64_lib())
    fptr = C.cast(UL.user_pad8_residual_d, C.c_void_p).value

    class Ctx(C.Structure):
        _fields_ = [("t", C.c_void_p), ("data", C.c_void_p), ("stream", C.c_void_p)]
    L = api.lib()
    st = api.Stream()
    dt_ = api.DeviceBuffer(t)
    lo = np.full(n, -np.inf); up = np.full(n, np.inf)
    loose = []
    for k in range(count):
        dd = api.DeviceBuffer(data[k])
        ctx = Ctx(dt_.ptr, dd.ptr, st.handle)
        go = api.GpuOptions(flags=M.DEVICE_CALLBACKS, stream=st.handle)
        xg = x0[k].copy()
        rg = L.mir_optimize_least_squares_gpu_d(C.byref(M.LeastSquaresSettings(np.float64)), t.size, n, xg.ctypes.data,
                                                lo.ctypes.data, up.ctypes.data, C.byref(go), C.addressof(ctx), fptr,
                                                None, None, None, None)
        dd.free()
        assert rg.status >= 0, (k, rg.status)
        agree(k, res[k], x[k], rg, xg, loose)
    dt_.free()
    assert len(loose) <= 1, loose
