"""Bounded problems finished INSIDE the batched one-wavefront-per-problem kernel (MIR_LSQ_BATCHED_DEVICE_BOUNDS, the bounded
instances k_lm_batched<Model, WEIGHTED, BatchedBoxQpStep> of csrc/batched_bounded.h, launch_batched_bounded<Model>), on the GPU.

Problem families (all seeded through problems.splitmix64_uniform):
  B3  bounded_problems() of tests/test_gpu_batched_f64.py restated: EXP_DECAY, 32 problems, m = 512, p1 >= 1.5; the bound binds on
      the even problems and stays far away on the odd ones.
  B8  the make_pad8 formulas with seeds 900 + k, 32 problems, m = 70 (no multiple of the wave) and m = 512, in the box
      lower = (-inf, 1, 0, -.1, -.1, -.1, -.1, -inf), upper = (inf, 2, inf, .1, .1, .1, .1, inf), the start clipped into it.
      With the oracle alone (CPU): every problem ends with status 0 or 1 in float and in double at both m, and between 1 and 5
      parameters finish exactly on a bound (m = 70: 2 / 5 / 7 / 15 / 3 problems with 1 .. 5), lower and upper bounds alike.
  U   unbounded controls: 16 problems each of make_exp_decay and make_pad8 as tests/test_gpu_batched_f64.py generates them.

The structural tests compare BITS (no tolerance): a problem whose steps stay inside the box takes the steps of the default
instance; the ladder, per-problem abscissae, a repeated launch and zero-weight padding change nothing.

The parity bars are the project's, not the new code's:
  double  `agree` of tests/test_gpu_batched_f64.py restated: the same status class on every problem, residual to 1e-9 and x to
          1e-6 on at least 95 % of the problems, the rest within 1e-7 / 1e-3;
  float   B3: the bar of test_batched_bounded_problems_fall_back_to_general_solver (x rtol 5e-3, atol 5e-4; residual rtol 5e-3);
          B8: the bar of test_cfg5_pad8_all_4096_problems_match_the_float_oracle (residual rtol 1e-3,
          |x - x_oracle| <= 5e-2 max(1, |x|)). The float and the double ORACLE differ on B8 by up to 3.6e-3 in a parameter and
          9e-5 in the residual, which is why the tighter EXP_DECAY bar is not used there.
Iteration and evaluation counts are not compared with the oracle or with the general solver: the docstring of
tests/test_gpu_batched_f64.py gives the reason. Every comparison prints its figures before it asserts.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import problems as P

pytestmark = pytest.mark.gpu

BOUNDS = M.BATCHED_DEVICE_BOUNDS
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
B8_LOWER = np.array([-np.inf, 1.0, 0.0, -0.1, -0.1, -0.1, -0.1, -np.inf])
B8_UPPER = np.array([np.inf, 2.0, np.inf, 0.1, 0.1, 0.1, 0.1, np.inf])


def rdt(dtype):
    f = "<f4" if dtype == np.float32 else "<f8"
    return np.dtype([("status", "<i4"), ("iterations", "<u4"), ("fCalls", "<u4"), ("gCalls", "<u4"), ("residual", f), ("lambda", f)])


def suffix(dtype):
    return "s" if dtype == np.float32 else "d"


# ---------------------------------------------------------------------------------------------------------------- families
def pad8_basis(t):
    return np.stack([np.sin(2 * t), np.cos(2 * t), np.sin(5 * t), np.cos(5 * t), t])


def make_pad8(count, m, seed0, noise=0.01):
    """make_pad8 of tests/test_gpu_batched_f64.py with the per-problem seed seed0 + k"""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 8))
    basis = pad8_basis(t)
    for k in range(count):
        u = P.splitmix64_uniform(seed0 + k, m + 16)
        p = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2], 0.6 * u[3] - 0.3, 0.6 * u[4] - 0.3, 0.6 * u[5] - 0.3,
                      0.6 * u[6] - 0.3, 0.1 * u[7] - 0.05])
        data[k] = p[0] * np.exp(-t * p[1]) + p[2] + p[3:] @ basis + noise * (2 * u[16:] - 1)
        x0[k] = p
        x0[k, :2] *= 1 + 0.2 * (2 * u[8:10] - 1)
        x0[k, 2:] += 0.1 * (2 * u[10:16] - 1)
    return t, data, x0


def make_exp_decay(count, m=512):
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 3))
    for k in range(count):
        u = P.splitmix64_uniform(100 + k, m + 6)
        truth = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2]])
        data[k] = truth[0] * np.exp(-t * truth[1]) + truth[2] + 0.01 * (2 * u[6:] - 1)
        x0[k] = truth * (1 + 0.3 * (2 * u[3:6] - 1))
    return t, data, x0


@functools.lru_cache(maxsize=None)
def family(name, m=512):
    """(model, t, data, x0, lower, upper) in float64; the arrays are shared by the tests and never written"""
    if name == "B3":
        count = 32
        t = np.linspace(0.0, 4.0, m)
        data = np.empty((count, m)); x0 = np.empty((count, 3))
        for k in range(count):
            u = P.splitmix64_uniform(700 + k, m + 6)
            p = np.array([1.0 + u[0], (0.8 if k % 2 == 0 else 2.0) + 0.4 * u[1], 0.2 * u[2]])
            data[k] = p[0] * np.exp(-t * p[1]) + p[2] + 0.01 * (2 * u[6:] - 1)
            x0[k] = p * (1 + 0.03 * (2 * u[3:6] - 1))
            if k % 2 == 0:
                x0[k, 1] = 1.7
        out = (M.MODEL_EXP_DECAY, t, data, x0, np.array([-np.inf, 1.5, -np.inf]), np.full(3, np.inf))
    elif name == "B8":
        t, data, x0 = make_pad8(32, m, 900)
        out = (M.MODEL_EXP_DECAY_PAD8, t, data, np.clip(x0, B8_LOWER, B8_UPPER), B8_LOWER, B8_UPPER)
    elif name == "U3":
        t, data, x0 = make_exp_decay(16, m)
        out = (M.MODEL_EXP_DECAY, t, data, x0, np.full(3, -np.inf), np.full(3, np.inf))
    elif name == "U8":
        t, data, x0 = make_pad8(16, m, 100)
        out = (M.MODEL_EXP_DECAY_PAD8, t, data, x0, np.full(8, -np.inf), np.full(8, np.inf))
    else:
        raise KeyError(name)
    for a in out[1:]:
        a.setflags(write=False)
    return out


BOUNDED_FAMILIES = [pytest.param("B3", 512, id="B3"), pytest.param("B8", 70, id="B8-m70"), pytest.param("B8", 512, id="B8-m512")]


def model_value(model, t, p):
    """in the precision of its arguments"""
    if model == M.MODEL_EXP_DECAY:
        return p[0] * np.exp(-t * p[1]) + p[2]
    return (p[0] * np.exp(-t * p[1]) + p[2] + p[3] * np.sin(2 * t) + p[4] * np.cos(2 * t) + p[5] * np.sin(5 * t)
            + p[6] * np.cos(5 * t) + p[7] * t)


_ORACLE = {}


def oracle_fits(oracle, name, m, dtype, qp_max_iterations=0):
    """the oracle's fit of every problem of a family in `dtype` (a Python f evaluating the model in that precision), computed
    once a session: [(result, x)]"""
    key = (name, m, np.dtype(dtype).name, qp_max_iterations)
    if key not in _ORACLE:
        model, t, data, x0, lo, up = family(name, m)
        tt = t.astype(dtype)
        out = []
        for k in range(x0.shape[0]):
            d = data[k].astype(dtype)

            def f(p, y):
                y[:] = model_value(model, tt, p) - d
            s = oracle.default_settings(dtype)
            s.qpSettings.maxIterations = qp_max_iterations
            out.append(oracle.optimize(f, m, x0[k].astype(dtype), lower=lo, upper=up, settings=s, dtype=dtype))
        _ORACLE[key] = out
    return _ORACLE[key]


# ----------------------------------------------------------------------------------------------------------------- launches
def run_kernel(dtype, model, x0, t, data, lo, up, variant=0, settings=None, weights=None, reps=1, fn=None):
    """mir_lsq_batched_kernel_s / _d (with weights: _ex_s / _ex_d) on device data with a caller-owned basis table -- or, with
    `fn`, a user library's entry of the same signature without the model id. Returns [(records, x)] per launch."""
    count, n = x0.shape
    m = data.shape[1]
    x0, t, data, lo, up = (np.ascontiguousarray(a, dtype=dtype) for a in (x0, t, data, lo, up))
    s = settings or M.LeastSquaresSettings(dtype)
    item = np.dtype(dtype).itemsize
    R = rdt(dtype)
    t_stride = 0 if t.ndim == 1 else m
    bufs = [api.DeviceBuffer(a) for a in (t, data, x0, lo, up)]
    dt_, dd, dx, dlo, dup = bufs
    dres = api.DeviceBuffer(nbytes=count * R.itemsize, dtype=np.uint8, shape=(count * R.itemsize,))
    rows = (count if t_stride else 1) * m
    dbasis = api.DeviceBuffer(nbytes=rows * 4 * item, dtype=dtype, shape=(rows, 4))
    st = api.Stream()
    opt = api.BatchedOptions(stream=st.handle, basis=dbasis.ptr, basis_bytes=rows * 4 * item, variant=variant)
    tail = [dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr, dres.ptr, C.byref(opt)]
    if fn is not None:
        head = [C.byref(s), count, m]
    elif weights is None:
        fn = getattr(api.lib(), "mir_lsq_batched_kernel_" + suffix(dtype))
        head = [C.byref(s), count, m, int(model)]
    else:
        fn = getattr(api.lib(), "mir_lsq_batched_kernel_ex_" + suffix(dtype))
        head = [C.byref(s), count, m, int(model)]
        weights = np.ascontiguousarray(weights, dtype=dtype)
        dw = api.DeviceBuffer(weights)
        bufs.append(dw)
        ex = api.BatchedExtras(weights=dw.ptr, weight_stride=0 if weights.ndim == 1 else m)
        tail.append(C.byref(ex))
    outs = []
    for _ in range(reps):
        dx.upload(x0)
        rc = fn(*head, *tail)
        assert rc == 0, rc
        st.synchronize()
        outs.append((np.frombuffer(dres.download().tobytes(), dtype=R).copy(), dx.download().reshape(count, n).copy()))
    for b in bufs + [dres, dbasis]:
        b.free()
    return outs


def same_bits(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def host_records(res, dtype):
    """the records of the Python host entry in the layout of the kernel entry's"""
    out = np.zeros(len(res), dtype=rdt(dtype))
    for k, r in enumerate(res):
        out[k] = (int(r.status), r.iterations, r.fCalls, r.gCalls, r.residual, r.lambda_)
    return out


# -------------------------------------------------------------------------------------------------------------- parity bars
def agree(k, status, residual, x, rr, xr, loose):
    """`agree` of tests/test_gpu_batched_f64.py (parameters, not curves) for one problem against the reference rr, xr"""
    assert (status >= 0) == (rr.status >= 0), (k, status, rr.status)
    if rr.status < 0:
        return 0.0, 0.0
    tight = np.allclose(x, xr, rtol=1e-6, atol=1e-7)
    near = np.allclose(x, xr, rtol=1e-3, atol=1e-4)
    gap = float(np.max(np.abs(x - xr) / np.maximum(np.abs(xr), 1e-3)))
    rgap = abs(residual / rr.residual - 1)
    if not (tight and rgap <= 1e-9):
        loose.append((k, gap, rgap))
        assert near and rgap <= 1e-7, (k, gap, rgap, x, xr)
    return gap, rgap


def compare_f64(label, raw, x, ref):
    """bar (9): ref = [(result, x)] per problem"""
    loose = []
    gaps = [agree(k, int(raw["status"][k]), float(raw["residual"][k]), x[k], rr, xr, loose) for k, (rr, xr) in enumerate(ref)]
    print(f"{label}: worst x gap {max(g for g, _ in gaps):.3e}, worst residual gap {max(r for _, r in gaps):.3e}, "
          f"{len(loose)} of {len(ref)} outside the tight bar: {loose}")
    assert len(loose) <= 0.05 * len(ref), loose


def compare_f32(label, name, raw, x, ref):
    """bar (10)"""
    st_o = np.array([int(r.status) for r, _ in ref]); res_o = np.array([float(r.residual) for r, _ in ref])
    xo = np.array([xk for _, xk in ref], dtype=np.float64)
    assert np.array_equal(raw["status"] >= 0, st_o >= 0), (raw["status"], st_o)
    ok = st_o >= 0
    x = x.astype(np.float64); resid = raw["residual"].astype(np.float64)
    rgap = np.abs(resid[ok] / res_o[ok] - 1)
    err = (np.abs(x - xo) / np.maximum(1.0, np.abs(xo))).max(axis=1)[ok]
    print(f"{label}: residual gap max {rgap.max():.3e}; |x - x_oracle| / max(1, |x|) max {err.max():.3e}, "
          f"|x - x_oracle| max {np.abs(x - xo)[ok].max():.3e}")
    if name == "B3":
        assert np.allclose(x[ok], xo[ok], rtol=5e-3, atol=5e-4) and np.allclose(resid[ok], res_o[ok], rtol=5e-3, atol=0)
    else:
        assert np.allclose(resid[ok], res_o[ok], rtol=1e-3, atol=0) and err.max() <= 5e-2


# ------------------------------------------------------------------------------------------- 1: the kernel entry, structural
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name, m", BOUNDED_FAMILIES)
def test_kernel_entry_with_the_bit_finishes_every_bounded_problem(oracle, name, m, dtype):
    """With the bit no problem comes back with -100 and every status is >= 0 (the oracle's is, on all 32); the parameters lie in
    the box, and one that the oracle leaves ON a bound IS that bound. Without the bit the entry answers as it always did: -100
    on the problems whose step reaches a bound (B3: the even ones) -- and the others took no bounded step, so the two instances
    give them the same bits."""
    model, t, data, x0, lo, up = family(name, m)
    ref = oracle_fits(oracle, name, m, dtype)
    assert all(r.status >= 0 for r, _ in ref), [int(r.status) for r, _ in ref]
    (raw, x), = run_kernel(dtype, model, x0, t, data, lo, up, variant=BOUNDS)
    print(f"{name} m={m} {np.dtype(dtype).name}: statuses {np.unique(raw['status'], return_counts=True)}")
    assert np.all(raw["status"] >= 0), raw["status"]
    lo_t, up_t = lo.astype(dtype), up.astype(dtype)
    assert np.all(x >= lo_t) and np.all(x <= up_t)
    xo = np.array([xk for _, xk in ref])
    on_lo, on_up = xo == lo_t, xo == up_t
    per_problem = (on_lo | on_up).sum(axis=1)
    print(f"   parameters the oracle leaves on a bound, per problem: {np.bincount(per_problem)} (lower {on_lo.sum()}, upper {on_up.sum()})")
    assert per_problem[0::2].min() >= 1 if name == "B3" else per_problem.min() >= 1
    assert np.all(x[on_lo] == np.broadcast_to(lo_t, x.shape)[on_lo]) and np.all(x[on_up] == np.broadcast_to(up_t, x.shape)[on_up])
    (raw0, x_0), = run_kernel(dtype, model, x0, t, data, lo, up)
    needs = raw0["status"] == -100
    print(f"   without the bit: -100 on {int(needs.sum())} problems")
    if name == "B3":
        assert np.array_equal(np.flatnonzero(needs), np.arange(0, 32, 2))
    else:
        assert needs.any()
    assert raw0[~needs].tobytes() == raw[~needs].tobytes() and x_0[~needs].tobytes() == x[~needs].tobytes()


# ------------------------------------------------------------------------------------------------- 2: never-binding bounds
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights-of-ones"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["U3", "U8", "B3-odd"])
def test_bounds_that_never_bind_give_the_bits_of_the_default_instance(name, dtype, weighted):
    """x, status, iterations, fCalls, gCalls, residual and lambda, bit for bit: the bounded instance with infinite bounds, and
    with finite bounds a factor 100 away from anything the fit visits, against the default instance."""
    if name == "B3-odd":
        model, t, data, x0, lo, up = family("B3")
        data, x0 = data[1::2], x0[1::2]
        boxes = [(lo, up)]                                  # p1 >= 1.5 stays far away on the odd problems
    else:
        model, t, data, x0, lo, up = family(name)
        far = 100 * (1 + np.abs(x0).max(axis=0))
        boxes = [(lo, up), (-far, far)]
    w = np.ones(t.size) if weighted else None
    for lo_k, up_k in boxes:
        base, = run_kernel(dtype, model, x0, t, data, lo_k, up_k, weights=w)
        with_bit, = run_kernel(dtype, model, x0, t, data, lo_k, up_k, weights=w, variant=BOUNDS)
        assert np.all(base[0]["status"] >= 0) and base[0]["iterations"].sum() > 2 * x0.shape[0]
        assert same_bits(base, with_bit)
    if len(boxes) == 2:                                     # and the far box changes nothing either
        inf_box, = run_kernel(dtype, model, x0, t, data, lo, up, weights=w, variant=BOUNDS)
        assert same_bits(inf_box, with_bit)


# ------------------------------------------------------------------------------------------------------------ 3: the ladder
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name, m", BOUNDED_FAMILIES)
def test_ladder_and_one_by_one_loop_give_the_same_bits_on_bounded_problems(name, m, dtype):
    model, t, data, x0, lo, up = family(name, m)
    a, = run_kernel(dtype, model, x0, t, data, lo, up, variant=BOUNDS)
    b, = run_kernel(dtype, model, x0, t, data, lo, up, variant=BOUNDS | M.BATCHED_NO_LADDER)
    assert same_bits(a, b)
    assert a[0]["iterations"].sum() > x0.shape[0]


# -------------------------------------------------------------------------------------------------------- 4: repeatability
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [70, 512])
def test_repeated_launch_own_abscissae_and_zero_weight_padding_change_no_bit(m, dtype):
    model, t, data, x0, lo, up = family("B8", m)
    count = x0.shape[0]
    first, second = run_kernel(dtype, model, x0, t, data, lo, up, variant=BOUNDS, reps=2)
    assert same_bits(first, second)
    own_t, = run_kernel(dtype, model, x0, np.tile(t, (count, 1)), data, lo, up, variant=BOUNDS)
    assert same_bits(first, own_t)
    # per-row weights, then the same problems with nine more rows of weight zero (finite data and abscissae there)
    w = 0.5 + P.splitmix64_uniform(77, m)
    weighted, = run_kernel(dtype, model, x0, t, data, lo, up, variant=BOUNDS, weights=w)
    assert not same_bits(first, weighted)
    t_pad = np.concatenate([t, 4.0 + 0.1 * np.arange(1, 10)])
    data_pad = np.concatenate([data, np.full((count, 9), 0.25)], axis=1)
    padded, = run_kernel(dtype, model, x0, t_pad, data_pad, lo, up, variant=BOUNDS, weights=np.concatenate([w, np.zeros(9)]))
    assert same_bits(weighted, padded)


# ------------------------------------------------------------------------------------------------------- 5: the host entry
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entry_with_the_bit_returns_the_kernel_entrys_results_and_finite_covariances(dtype):
    """no fallback ran: the records (fCalls included) and x are the kernel's, bit for bit; and the covariance kernel runs on them"""
    model, t, data, x0, lo, up = family("B8", 512)
    (raw, x), = run_kernel(dtype, model, x0, t, data, lo, up, variant=BOUNDS)
    res, xh = M.optimizeLeastSquaresBatched(model, x0, t, data, l=lo, u=up, variant=BOUNDS, dtype=dtype)
    assert host_records(res, dtype).tobytes() == raw.tobytes() and xh.tobytes() == x.tobytes()
    res, xc, cov = M.optimizeLeastSquaresBatched(model, x0, t, data, l=lo, u=up, variant=BOUNDS, dtype=dtype, covariance=True)
    assert host_records(res, dtype).tobytes() == raw.tobytes() and xc.tobytes() == x.tobytes()
    assert cov.shape == (32, 8, 8) and np.all(np.isfinite(cov))
    assert np.all(np.diagonal(cov, axis1=1, axis2=2) > 0)


# ------------------------------------------------------------------------------------------- 6: a QP that runs out of steps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [70, 512])
def test_qp_iteration_limit_of_one_ends_like_the_reference(oracle, m, dtype):
    """qpSettings.maxIterations = 1: a box QP that is not solved after one active-set step ends the fit with numericError
    (-26, LS:1080-1085). Every status is >= 0 or -26 and of the oracle's class for the same settings. The only test that may
    see -26."""
    model, t, data, x0, lo, up = family("B8", m)
    s = M.LeastSquaresSettings(dtype)
    s.qpSettings.maxIterations = 1
    (raw, x), = run_kernel(dtype, model, x0, t, data, lo, up, variant=BOUNDS, settings=s)
    st_o = np.array([int(r.status) for r, _ in oracle_fits(oracle, "B8", m, dtype, qp_max_iterations=1)])
    print(f"B8 m={m} {np.dtype(dtype).name}, qp maxIterations 1: kernel {raw['status'].tolist()}\n   oracle {st_o.tolist()}")
    assert np.all((raw["status"] >= 0) | (raw["status"] == -26)), raw["status"]
    assert np.array_equal(raw["status"] >= 0, st_o >= 0)


# ---------------------------------------------------------------------------------------------------- 7: the header entry
def user_entry(name):
    """an entry of tests/user_model/libuser_model_bounded.so with its C signature declared"""
    fn = getattr(C.CDLL(hipbuild.user_model_bounded_lib()), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                   C.c_void_p, C.c_void_p]
    return fn


CAPACITY = 2.0


def logistic_problems(count=16, m=200):
    """the caller's model of tests/user_model/user_model_bounded.hip, p0 / (1 + exp(-p1 (t - p2))) + p3, with the capacity
    bounded from above: p0 <= 2 cuts the minimiser off (true p0 = 2.0 .. 2.1) on every problem, in float and in double"""
    t = np.linspace(0.0, 10.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 4))
    for k in range(count):
        u = P.splitmix64_uniform(1300 + k, m + 8)
        p = np.array([2.0 + 0.1 * u[0], 0.8 + 0.4 * u[1], 4.5 + u[2], 0.1 * u[3]])
        data[k] = p[0] / (1 + np.exp(-p[1] * (t - p[2]))) + p[3] + 0.01 * (2 * u[8:] - 1)
        x0[k] = p * (1 + 0.05 * (2 * u[4:8] - 1))
        x0[k, 0] = min(x0[k, 0], CAPACITY) - 0.05
    return t, data, x0, np.full(4, -np.inf), np.array([CAPACITY, np.inf, np.inf, np.inf])


@pytest.mark.parametrize("dtype", DTYPES)
def test_user_model_through_launch_batched_bounded_matches_the_oracle(oracle, dtype):
    """double: bar (9). float: every problem is finished and the bound binds exactly, as in the float oracle; its figures against
    the float oracle are printed, not asserted: the project has no float bar for this family, whose constrained valley is flat
    in float (the float and the double ORACLE already differ by 2.5e-3 in a parameter and 5.5e-4 in the residual; measured on
    the device against the float oracle: 2.7e-3 and 4.1e-3)."""
    t, data, x0, lo, up = logistic_problems()
    (raw, x), = run_kernel(dtype, None, x0, t, data, lo, up, fn=user_entry("user_fit_logistic_bounded_" + suffix(dtype)))
    assert np.all(raw["status"] >= 0), raw["status"]
    assert np.all(x[:, 0] == dtype(CAPACITY))              # the bound binds
    tt = t.astype(dtype)
    ref = []
    for k in range(x0.shape[0]):
        d = data[k].astype(dtype)

        def f(p, y):
            y[:] = p[0] / (1 + np.exp(-p[1] * (tt - p[2]))) + p[3] - d
        ref.append(oracle.optimize(f, t.size, x0[k].astype(dtype), lower=lo, upper=up, dtype=dtype))
    assert all(r.status >= 0 and xk[0] == dtype(CAPACITY) for r, xk in ref)
    if dtype == np.float64:
        compare_f64("user model, launch_batched_bounded", raw, x, ref)
    else:
        res_o = np.array([float(r.residual) for r, _ in ref])
        xo = np.array([xk for _, xk in ref], dtype=np.float64)
        print(f"user model f32: residual gap max {np.abs(raw['residual'] / res_o - 1).max():.3e}, |x - x_oracle| max "
              f"{np.abs(x - xo).max():.3e} (not asserted)")


def test_launch_batched_refuses_the_bit_and_keeps_its_default_instance():
    t, data, x0, lo, up = logistic_problems()
    fit = user_entry("user_fit_logistic_d")
    (raw, _), = run_kernel(np.float64, None, x0, t, data, lo, up, fn=fit)
    assert np.all(raw["status"] == -100)                   # the default instance of the caller's model: as always
    s = M.LeastSquaresSettings(np.float64)
    bufs = [api.DeviceBuffer(np.ascontiguousarray(a)) for a in (x0, lo, up, t, data)]
    dres = api.DeviceBuffer(nbytes=16 * 32, dtype=np.uint8, shape=(16 * 32,))
    opt = api.BatchedOptions(variant=BOUNDS)
    rc = fit(C.byref(s), 16, t.size, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 0, bufs[4].ptr, dres.ptr, C.byref(opt))
    for b in bufs + [dres]:
        b.free()
    assert rc == -1


# ------------------------------------------------------------------------------------------------------- 9, 10, 11: parity
def default_path(dtype, name, m):
    """the host entry WITHOUT the bit: the general solver finishes the -100 problems"""
    model, t, data, x0, lo, up = family(name, m)
    res, x = M.optimizeLeastSquaresBatched(model, x0, t, data, l=lo, u=up, dtype=dtype)
    return host_records(res, dtype), x


@pytest.mark.parametrize("name, m", BOUNDED_FAMILIES)
def test_f64_bounded_fits_match_the_bounded_oracle(oracle, name, m):
    """bar (9) for the new path, and for the default path (the general solver) on the same family through the same comparison"""
    model, t, data, x0, lo, up = family(name, m)
    ref = oracle_fits(oracle, name, m, np.float64)
    (raw, x), = run_kernel(np.float64, model, x0, t, data, lo, up, variant=BOUNDS)
    raw_d, x_d = default_path(np.float64, name, m)
    try:
        compare_f64(f"{name} m={m} f64, default path (general solver)", raw_d, x_d, ref)
    finally:
        compare_f64(f"{name} m={m} f64, in-kernel bounded step", raw, x, ref)


@pytest.mark.parametrize("name, m", BOUNDED_FAMILIES)
def test_f32_bounded_fits_match_the_bounded_float_oracle(oracle, name, m):
    """bar (10), the new path and the default path"""
    model, t, data, x0, lo, up = family(name, m)
    ref = oracle_fits(oracle, name, m, np.float32)
    (raw, x), = run_kernel(np.float32, model, x0, t, data, lo, up, variant=BOUNDS)
    raw_d, x_d = default_path(np.float32, name, m)
    try:
        compare_f32(f"{name} m={m} f32, default path (general solver)", name, raw_d, x_d, ref)
    finally:
        compare_f32(f"{name} m={m} f32, in-kernel bounded step", name, raw, x, ref)


@pytest.mark.parametrize("m", [70, 512])
def test_f64_in_kernel_bounded_step_agrees_with_the_default_path(m):
    """(11): B8 in double with the bit against the host entry without it, at bar (9)"""
    model, t, data, x0, lo, up = family("B8", m)
    (raw, x), = run_kernel(np.float64, model, x0, t, data, lo, up, variant=BOUNDS)
    raw_d, x_d = default_path(np.float64, "B8", m)

    class R:
        def __init__(self, rec):
            self.status, self.residual = int(rec["status"]), float(rec["residual"])
    compare_f64(f"B8 m={m} f64, in-kernel bounded step against the default path", raw, x, [(R(raw_d[k]), x_d[k]) for k in range(32)])
