"""The batched one-wavefront-per-problem fit for models with 9 to 16 parameters (k_lm_batched16: csrc/batched16_kernel.h;
mir_optimize_least_squares_batched16_d, mir_lsq_batched16_kernel_d, launch_batched16<Model>) against the oracle's double
instantiation, problem by problem, at the project's f64 parity bar (tests/test_gpu_batched_f64.py): same status class on every
problem, residual to rtol 1e-9 and x to rtol 1e-6 / atol 1e-7 on at least 95 % of them, every problem within rtol 1e-7 on the
residual and 1e-3 / 1e-4 on x. The kernel sums J^T J on the matrix unit and evaluates exp / sin / cos with the device library,
the oracle sums sequentially with numpy's functions: counts of iterations and evaluations are not compared, minima are.
The oracle against ITSELF with the rows reversed (another summation order) stays inside this bar on these inputs.

The harmonic family: t = linspace(0, 4, m); p0 exp(-t p1) + p2 + sum_j p_j h_j(t) with h_j = sin / cos(k pi / 2 t) for odd /
even j, k = (j - 1) // 2; 64 problems a case, truth, start and noise from splitmix64_uniform(700 + k, m + 2 n). n = 9 and 13 are
a caller's own models (tests/user_model/user_model_n16.hip, through the public device header: padded columns of the 16-wide
tile), n = 16 is the built-in MIR_LSQ_MODEL16_EXP_HARM16. m = 2 n + 1 (fewer rows than lanes), 67 (m % 4 != 0, two row chunks
per lane) and 130 (three)."""
import ctypes as C
import functools

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
from batched16_problems import COUNT, RDT, gauss3_problems, gauss3_value, harm_problems, harm_value     # shared with scripts/batched16.py

pytestmark = pytest.mark.gpu

MAX_ROWS = 1119            # (16 + 2) m + 272 doubles <= 160 KB - 512
ANALYTIC = 2               # MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN


_ORACLE = {}


def oracle_harm(oracle, n, m, analytic=False, box=None, reverse=False, count=COUNT):
    """the oracle's fits of harm_problems(n, m), computed once and shared: [(result, x)]. box: (lower, upper, starts)"""
    key = (n, m, analytic, box is not None, reverse, count)
    if key not in _ORACLE:
        t, B, data, truth, x0 = harm_problems(n, m, count)
        lo, up, starts = box if box is not None else (None, None, x0)
        if reverse:
            t, B, data = t[::-1].copy(), B[:, ::-1].copy(), data[:, ::-1].copy()
        out = []
        for k in range(count):
            def f(p, y, d=data[k]):
                y[:] = harm_value(B, t, p) - d

            def g(p, J):
                e = np.exp(-t * p[1])
                J[:, 0] = e; J[:, 1] = -t * p[0] * e; J[:, 2] = 1.0; J[:, 3:] = B.T
            out.append(oracle.optimize(f, m, starts[k], lower=lo, upper=up, g=g if analytic else None, dtype=np.float64))
        _ORACLE[key] = out
    return _ORACLE[key]


def gaps(r, x, rr, xr):
    """(tight, near, figures) of one problem against its reference at the bar of this file"""
    tight = np.allclose(x, xr, rtol=1e-6, atol=1e-7)
    near = np.allclose(x, xr, rtol=1e-3, atol=1e-4)
    gap = float(np.max(np.abs(x - xr) / np.maximum(np.abs(xr), 1e-3)))
    rgap = abs(r.residual / rr.residual - 1)
    return tight and rgap <= 1e-9, near and rgap <= 1e-7, (gap, rgap)


def compare(res, x, ref, loose_ok=0.05, skip=()):
    loose = []
    for k, (rr, xr) in enumerate(ref):
        assert (res[k].status >= 0) == (rr.status >= 0), (k, res[k].status, rr.status)
        assert res[k].status != -100, k
        if rr.status < 0 or k in skip:
            continue
        tight, near, fig = gaps(res[k], x[k], rr, xr)
        if not tight:
            loose.append((k,) + fig)
        assert near, (k, fig, x[k], xr)
    print(f"loose {len(loose)} of {len(ref) - len(skip)}: {loose}")
    assert len(loose) <= loose_ok * (len(ref) - len(skip)), loose
    return loose


class Rec:
    """a result record of the kernel entries with the attributes of LeastSquaresResult"""
    def __init__(self, row):
        self.status, self.iterations, self.fCalls, self.gCalls = int(row["status"]), int(row["iterations"]), int(row["fCalls"]), int(row["gCalls"])
        self.residual, self.lambda_ = float(row["residual"]), float(row["lambda"])


def run_device(fn, x0, t, data, lo=None, up=None, variant=0, model=None, reps=1, rc_expected=0):
    """a device-pointer entry on device data: mir_lsq_batched16_kernel_d (model given) or a user library's entry; the basis
    table is the call's own. Returns [(records, x)] per launch"""
    count, n = x0.shape
    m = data.shape[1]
    s = M.LeastSquaresSettings(np.float64)
    lo = np.full(n, -np.inf) if lo is None else lo
    up = np.full(n, np.inf) if up is None else up
    t_stride = 0 if t.ndim == 1 else m
    bufs = [api.DeviceBuffer(np.ascontiguousarray(a)) for a in (t, data, x0, lo, up)]
    dt_, dd, dx, dlo, dup = bufs
    dres = api.DeviceBuffer(nbytes=count * 32, dtype=np.uint8, shape=(count * 32,))
    st = api.Stream()
    opt = api.BatchedOptions(stream=st.handle, variant=variant)
    outs = []
    for _ in range(reps):
        dx.upload(np.ascontiguousarray(x0))
        args = [C.byref(s), count, m] + ([model] if model is not None else []) + [dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr,
                                                                                 dres.ptr, C.byref(opt)] + ([None] if model is not None else [])
        rc = fn(*args)
        assert rc == rc_expected, rc
        st.synchronize()
        outs.append((np.frombuffer(dres.download().tobytes(), dtype=RDT).copy(), dx.download().reshape(count, n).copy()))
    for b in bufs + [dres]:
        b.free()
    return outs


@functools.lru_cache(maxsize=None)
def user_lib():
    UL = C.CDLL(hipbuild.user_model_n16_lib())
    for name in ("user_fit_harm9_d", "user_fit_harm13_d"):
        fn = getattr(UL, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                       C.c_void_p, C.c_void_p]
    return UL


def fit_harm(n, x0, t, data, lo=None, up=None, variant=0):
    """n = 16: the built-in model through the host entry; n = 9, 13: the caller's models through the device header"""
    if n == 16:
        return M.optimizeLeastSquaresBatched(M.MODEL16_EXP_HARM16, x0, t, data, l=lo, u=up, variant=variant, dtype=np.float64)
    (raw, x), = run_device(getattr(user_lib(), f"user_fit_harm{n}_d"), x0, t, data, lo, up, variant)
    return [Rec(r) for r in raw], x


@pytest.mark.parametrize("m", ["2n+1", 67, 130])
@pytest.mark.parametrize("n", [9, 13, 16])
def test_harmonic_fits_match_the_f64_oracle(oracle, n, m):
    m = 2 * n + 1 if m == "2n+1" else m
    t, B, data, truth, x0 = harm_problems(n, m)
    res, x = fit_harm(n, x0, t, data)
    assert all(r.iterations >= 1 for r in res) and all(r.gCalls == 0 for r in res)
    compare(res, x, oracle_harm(oracle, n, m))


def test_gauss3_affine_matches_the_f64_oracle(oracle):
    t, data, x0 = gauss3_problems()
    res, x = M.optimizeLeastSquaresBatched(M.MODEL16_GAUSS3_AFFINE, x0, t, data, dtype=np.float64)
    ref = []
    for k in range(COUNT):
        def f(p, y, d=data[k]):
            y[:] = gauss3_value(t, p) - d
        ref.append(oracle.optimize(f, t.size, x0[k], dtype=np.float64))
    assert all(r.iterations >= 1 for r in res)
    compare(res, x, ref)
    with pytest.raises(RuntimeError, match="-1"):                       # the model has no derivative
        M.optimizeLeastSquaresBatched(M.MODEL16_GAUSS3_AFFINE, x0, t, data, dtype=np.float64, variant=ANALYTIC)


@pytest.mark.parametrize("n", [9, 13])
def test_analytic_jacobian_matches_the_oracle_with_g(oracle, n):
    m = 67
    t, B, data, truth, x0 = harm_problems(n, m)
    res, x = fit_harm(n, x0, t, data, variant=ANALYTIC)
    assert all(r.gCalls >= 1 for r in res)                                 # every refresh that is not a Broyden update is a g call
    compare(res, x, oracle_harm(oracle, n, m, analytic=True))


def boxed(n, m):
    """p3 .. p15 boxed to +- 0.25, the start clipped into the box; the other parameters unbounded"""
    t, B, data, truth, x0 = harm_problems(n, m)
    lo = np.full(n, -np.inf); up = np.full(n, np.inf)
    lo[3:] = -0.25; up[3:] = 0.25
    starts = np.clip(x0, lo, up)
    return t, B, data, lo, up, starts


@pytest.mark.parametrize("m", [67, 130])
def test_bounded_fits_finish_in_the_kernel_and_match_the_bounded_oracle(oracle, m):
    n = 16
    t, B, data, lo, up, starts = boxed(n, m)
    res, x = fit_harm(n, starts, t, data, lo, up)
    ref = oracle_harm(oracle, n, m, box=(lo, up, starts))
    again = oracle_harm(oracle, n, m, box=(lo, up, starts), reverse=True)
    on_bound = [int(np.sum((xr == lo) | (xr == up))) for _, xr in ref]
    assert sum(1 for c in on_bound if c >= 1) >= COUNT // 2, on_bound      # the box binds on most problems
    aside = set()
    for k, ((rr, xr), (r2, x2)) in enumerate(zip(ref, again)):
        assert (res[k].status >= 0) == (rr.status >= 0) and res[k].status != -100, (k, res[k].status, rr.status)
        assert np.all(x[k] >= lo) and np.all(x[k] <= up), k                # inside the box exactly
        if rr.status < 0:
            continue
        assert abs(res[k].residual / rr.residual - 1) <= 1e-6, (k, res[k].residual, rr.residual)
        if not gaps(r2, x2, rr, xr)[0]:
            aside.add(k)                                                   # the oracle's own two summation orders disagree here
    print(f"set aside {sorted(aside)}; parameters on a bound {on_bound}")
    assert len(aside) <= 0.10 * COUNT, sorted(aside)
    compare(res, x, ref, skip=aside)


def test_two_launches_on_device_data_give_the_same_bits():
    t, B, data, truth, x0 = harm_problems(16, 67)
    (r1, x1), (r2, x2) = run_device(api.lib().mir_lsq_batched16_kernel_d, x0, t, data, model=M.MODEL16_EXP_HARM16, reps=2)
    assert r1.tobytes() == r2.tobytes() and x1.tobytes() == x2.tobytes()
    assert np.all(r1["status"] >= 0) and r1["iterations"].sum() > 3 * COUNT


def test_per_problem_abscissae_give_the_bits_of_shared_ones():
    t, B, data, truth, x0 = harm_problems(16, 67)
    res0, xa = fit_harm(16, x0, t, data)
    res1, xb = fit_harm(16, x0, np.tile(t, (COUNT, 1)), data)
    assert (xa.view(np.uint64) == xb.view(np.uint64)).all()
    assert [(int(r.status), r.iterations, r.fCalls, r.residual) for r in res0] == [(int(r.status), r.iterations, r.fCalls, r.residual) for r in res1]
    t3 = np.tile(t, (COUNT, 1))
    t3[7] *= 1.01                                                       # problem 7 sees other abscissae
    res2, xc = fit_harm(16, x0, t3, data)
    same = (xa.view(np.uint64) == xc.view(np.uint64)).all(axis=1)
    assert same[np.arange(COUNT) != 7].all() and not same[7]


def test_infinite_bounds_give_the_bits_of_a_huge_finite_box():
    t, B, data, truth, x0 = harm_problems(16, 67)
    res0, xa = fit_harm(16, x0, t, data)
    res1, xb = fit_harm(16, x0, t, data, np.full(16, -1e300), np.full(16, 1e300))
    assert (xa.view(np.uint64) == xb.view(np.uint64)).all()
    assert [(int(r.status), r.iterations, r.fCalls, r.residual) for r in res0] == [(int(r.status), r.iterations, r.fCalls, r.residual) for r in res1]


def test_batched_fit_agrees_with_the_general_solver_on_the_same_model():
    """16 problems of the built-in 16-parameter model: the batched fit against mir_optimize_least_squares_gpu_d driven by a device
    callback of the same model (tests/user_model/user_model_n16.hip), at the bar of this file."""
    count, n, m = 16, 16, 67
    t, B, data, truth, x0 = harm_problems(n, m)
    res, x = fit_harm(n, x0[:count], t, data[:count])
    UL = user_lib()
    fptr = C.cast(UL.user_harm16_residual_d, C.c_void_p).value

    class Ctx(C.Structure):
        _fields_ = [("t", C.c_void_p), ("data", C.c_void_p), ("stream", C.c_void_p)]
    L = api.lib()
    st = api.Stream()
    dt_ = api.DeviceBuffer(np.ascontiguousarray(t))
    lo = np.full(n, -np.inf); up = np.full(n, np.inf)
    ref = []
    for k in range(count):
        dd = api.DeviceBuffer(np.ascontiguousarray(data[k]))
        ctx = Ctx(dt_.ptr, dd.ptr, st.handle)
        go = api.GpuOptions(flags=M.DEVICE_CALLBACKS, stream=st.handle)
        xg = x0[k].copy()
        rg = L.mir_optimize_least_squares_gpu_d(C.byref(M.LeastSquaresSettings(np.float64)), m, n, xg.ctypes.data, lo.ctypes.data,
                                                up.ctypes.data, C.byref(go), C.addressof(ctx), fptr, None, None, None, None)
        dd.free()
        assert rg.status >= 0, (k, rg.status)
        ref.append((rg, xg))
    dt_.free()
    compare(res, x, ref)                   # at least 95 % tight: on 16 problems, all of them


def test_limits_and_validation_codes(oracle):
    n = 16
    t, B, data, truth, x0 = harm_problems(n, 67)
    xn = np.array(x0[:4]); xn[1, 5] = np.nan; xn[2, 0] = np.inf
    res, _ = fit_harm(n, xn, t, data[:4])
    assert [int(r.status) for r in res][1:3] == [-31, -31] and res[0].status >= 0 and res[3].status >= 0
    lo = np.full(n, -np.inf); lo[4] = 5.0                                  # the start lies outside its bounds
    res, _ = fit_harm(n, x0[:4], t, data[:4], lo=lo)
    assert all(int(r.status) == -32 for r in res)
    # one above the documented row limit: -3 from both entries
    tb, Bb, db, _, xb = harm_problems(n, MAX_ROWS + 1, 1)
    with pytest.raises(RuntimeError, match="-3"):
        fit_harm(n, xb, tb, db)
    run_device(api.lib().mir_lsq_batched16_kernel_d, xb, tb, db, model=M.MODEL16_EXP_HARM16, rc_expected=-3)
    # ... and one problem at the limit itself (more than 48 KB of dynamic LDS) runs and matches the oracle
    tb, Bb, db, _, xb = harm_problems(n, MAX_ROWS, 1)
    res, x = fit_harm(n, xb, tb, db)
    ref = oracle_harm(oracle, n, MAX_ROWS, count=1)
    tight, near, fig = gaps(res[0], x[0], *ref[0])
    print("at the row limit:", fig)
    assert res[0].status >= 0 and ref[0][0].status >= 0 and tight, fig     # one problem: the tight bar


@pytest.mark.parametrize("n", [9, 16])
def test_jtj_stage_matches_numpy(n):
    """mir_lsq_batched16_jtj_d: the MFMA accumulation of J^T J and the J^T y that rides on it, against numpy in float64. The bound
    is 2 m eps sum_i |a_i b_i| per entry: the textbook bound m eps sum |a_i b_i| on a sum of m products in any order, once for
    each side. The tile is exactly symmetric; rows and columns >= n are exactly zero."""
    rng = np.random.default_rng(160 + n)
    eps = np.finfo(np.float64).eps
    for m in (1, 3, 4, 17, 67):
        count = 8
        J = rng.standard_normal((count, m, n)) * np.logspace(-2, 2, n)[None, None, :]
        y = rng.standard_normal((count, m))
        JJ, Jy = M.batched16JtJ(J, y)
        assert JJ.shape == (count, 16, 16) and Jy.shape == (count, 16)
        assert (JJ == JJ.transpose(0, 2, 1)).all(), m
        assert not JJ[:, n:, :].any() and not JJ[:, :, n:].any() and not Jy[:, n:].any(), m
        for p in range(count):
            ref = J[p].T @ J[p]
            bound = 2 * m * eps * (np.abs(J[p]).T @ np.abs(J[p]))
            err = np.abs(JJ[p, :n, :n] - ref)
            assert (err <= bound).all(), (m, p, float((err / bound).max()))
            refy = J[p].T @ y[p]
            boundy = 2 * m * eps * (np.abs(J[p]).T @ np.abs(y[p]))
            erry = np.abs(Jy[p, :n] - refy)
            assert (erry <= boundy).all(), (m, p, float((erry / boundy).max()))
