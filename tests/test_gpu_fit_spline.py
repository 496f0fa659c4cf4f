"""fitSpline on device-resident points, on the GPU: the residual kernels against their host twins (array_equal: one statement
of the arithmetic, csrc/spline_c2.h, correctly rounded operations, contraction off), the evaluation entry against
mir_spline_eval_*, and mir_fit_spline_gpu_* end to end against the reference's unittest (fit_splie.d:88-141), the oracle and
the host-callback entry. Inputs: tests/fit_spline_cases.py; tests/test_fit_spline_gpu_host.py has checked that the oracle
converges on every fit-level input, so no comparison here skips a case."""
import numpy as np
import pytest

import fit_spline_cases as K
import mir_optim_amd as M

pytestmark = pytest.mark.gpu

_oracle_cache = {}


def oracle_fit(oracle, pts, x, lam, lo=None, up=None):
    key = (pts.tobytes(), x.tobytes(), lam, None if lo is None else lo.tobytes(), None if up is None else up.tobytes())
    if key not in _oracle_cache:
        def f(v, y):
            y[:] = M.fit_spline_residuals(pts, x, lam, v)
        kw = {} if lo is None else dict(lower=lo, upper=up)
        _oracle_cache[key] = oracle.optimize(f, pts.shape[0] + (1 if lam == 0 else 0), np.zeros(x.size), **kw)
    return _oracle_cache[key]


def free(n):
    return np.full(n, -np.inf), np.full(n, np.inf)


# ---- 4. callback level
@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("nx", K.GRID_NX)
def test_callbacks_equal_their_host_twins(nx, family):
    x, cases = K.grid_cases(nx, family)
    for lam, pts, V in cases:
        tag = (nx, family, lam, pts.shape[0], V.shape[0])
        dev = M.DeviceBuffer(pts)
        assert np.array_equal(M.fit_spline_eval_gpu(dev, x, lam, V, mode=0), M.fit_spline_eval_host(pts, x, lam, V, mode=0)), tag
        assert np.array_equal(M.fit_spline_eval_gpu(dev, x, lam, V, mode=1), M.fit_spline_eval_host(pts, x, lam, V, mode=1)), tag
        dev.free()
        got = M.fit_spline_eval_gpu(pts, x, lam, V, mode=0, dtype=np.float32)
        assert np.array_equal(got, M.fit_spline_eval_host(pts, x, lam, V, mode=0, dtype=np.float32)), tag


def test_base_point_tail_is_the_point_major_vector():
    """MIR_LSQ_FD_BASE_POINT's promise: the residual vector behind the panel is, bit for bit, what f writes for that point."""
    x, cases = K.grid_cases(37, "pivoting")
    for lam, pts, V in cases:
        if V.shape[0] != 2 * 37 + 1:
            continue
        m = pts.shape[0] + (1 if lam == 0 else 0)
        D = M.fit_spline_eval_gpu(pts, x, lam, V, mode=1)
        assert np.array_equal(D[m * 37:], M.fit_spline_eval_gpu(pts, x, lam, V[-1:], mode=0)[0])


# ---- 5. evaluation entry
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nx", [1, 2, 3, 4, 37])
def test_spline_eval_gpu_equals_host_eval(nx, dtype):
    x = K.knots(nx, "uniform")
    s = M.Spline(x, np.random.default_rng(nx).normal(0.0, 2.0, nx), dtype)
    t = np.resize(K.abscissae(x, 50 + nx), 300).astype(dtype)
    ref = np.array([s.withTwoDerivatives(v)[0] for v in t], dtype=dtype)
    got = M.splineEvalGpu(s, t)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, ref)
    dt = M.DeviceBuffer(t)
    out = M.splineEvalGpu(s, dt)
    assert np.array_equal(out.download(), ref)


# ---- 6. the reference's unittest, double
@pytest.mark.parametrize("lam,expect", [(0.0, K.Y0), (1e-3, K.Y_LAMBDA)])
def test_reference_unittest(oracle, lam, expect):
    lo, up = free(10)
    st = M.Stats()
    r = M.fitSplineGpu(M.LeastSquaresSettings(), K.POINTS, K.X, lo, up, lam, stats=st)
    got = np.array([r.spline(t) for t in K.X])
    assert K.approx(got, expect), np.abs(got - expect).max()                   # FS:119-120, FS:140-141
    ro, vo = oracle_fit(oracle, K.POINTS, K.X, lam)
    lr = r.leastSquaresResult
    assert int(lr.status) == ro.status and np.allclose(r.spline.values, vo, rtol=1e-6, atol=1e-8)
    assert np.isclose(lr.residual, ro.residual, rtol=1e-9, atol=1e-12)
    if lam == 0:
        assert abs(lr.iterations - ro.iterations) <= 2
    assert st.jtj_fd_launches > 0 and st.fd_callback_calls > 0                 # the difference-panel path really ran
    assert np.array_equal(r.spline.derivatives, M.Spline(K.X, r.spline.values).derivatives)


# ---- 7. base point
@pytest.mark.parametrize("lam", [0.0, 1e-3])
def test_base_point_changes_nothing(oracle, lam):
    lo, up = free(10)
    a = M.fitSplineGpu(None, K.POINTS, K.X, lo, up, lam)
    b = M.fitSplineGpu(None, K.POINTS, K.X, lo, up, lam, variant=M.VARIANT_NO_FD_BASE_POINT)
    ra, rb = a.leastSquaresResult, b.leastSquaresResult
    assert np.array_equal(a.spline.values, b.spline.values)
    assert (ra.status, ra.iterations, ra.fCalls, ra.residual) == (rb.status, rb.iterations, rb.fCalls, rb.residual)
    st = M.Stats()
    c = M.fitSplineGpu(None, K.POINTS, K.X, lo, up, lam, variant=M.VARIANT_FD_SEPARATE_FILL, stats=st)
    ro, vo = oracle_fit(oracle, K.POINTS, K.X, lam)
    rc = c.leastSquaresResult
    assert st.jtj_fd_launches == 0 and st.fd_callback_calls > 0                # the fb path
    assert int(rc.status) == ro.status and np.allclose(c.spline.values, vo, rtol=1e-6, atol=1e-8)
    assert np.isclose(rc.residual, ro.residual, rtol=1e-9, atol=1e-12)
    if lam == 0:
        assert abs(rc.iterations - ro.iterations) <= 2


# ---- 8. bounds and errors
def test_bounds_and_errors(oracle):
    lo, up = np.zeros(10), np.full(10, 15.0)
    r = M.fitSplineGpu(None, K.POINTS, K.X, lo, up, 1e-3)
    v = r.spline.values
    assert np.all(v >= 0.0) and np.all(v <= 15.0) and np.sum(v == 15.0) >= 3
    ro, vo = oracle_fit(oracle, K.POINTS, K.X, 1e-3, lo, up)
    assert np.allclose(v, vo, rtol=1e-6, atol=1e-8)
    with pytest.raises(M.LeastSquaresException, match="[Bb]ound"):             # y = 0 outside [1, 15]
        M.fitSplineGpu(None, K.POINTS, K.X, lo + 1.0, up, 0.0)
    with pytest.raises(Exception, match="greater or equal"):                   # FS:47-51
        M.fitSplineGpu(None, K.POINTS[:5], K.X, *free(10), 0.0)
    dev = M.DeviceBuffer(K.POINTS[:5])
    with pytest.raises(Exception, match="greater or equal"):                   # the entry's own code, not the wrapper's check
        M.fitSplineGpu(None, dev, K.X, *free(10), 0.0)


# ---- 9. generated inputs against the host-callback entry
@pytest.mark.parametrize("case", K.generated_cases(), ids=lambda c: c[0])
def test_generated_inputs_against_host_path(case):
    name, pts, x, lam, lo, up = case
    st = M.Stats()
    g = M.fitSplineGpu(None, pts, x, lo, up, lam, stats=st)
    h = M.fitSpline(None, pts, x, lo, up, lam)
    rg, rh = g.leastSquaresResult, h.leastSquaresResult
    print(name, "max |dv|", np.abs(g.spline.values - h.spline.values).max(), "residuals", rg.residual, rh.residual,
          "iterations", rg.iterations, rh.iterations)
    assert K.approx(g.spline.values, h.spline.values), np.abs(g.spline.values - h.spline.values).max()
    assert np.isclose(rg.residual, rh.residual, rtol=1e-9, atol=0.0)
    assert rg.status >= 0 and rh.status >= 0
    assert st.fd_callback_calls > 0
    if x.size == 130:
        assert st.jtj_fd_launches == 0          # no difference-panel J^T J kernel at n = 130: the solver takes fb + fill by itself
    else:
        assert st.jtj_fd_launches > 0


# ---- 10. float
def test_reference_unittest_float():
    lo, up = free(10)
    r = M.fitSplineGpu(M.LeastSquaresSettings(np.float32), K.POINTS, K.X, lo, up, 0.0, dtype=np.float32)
    assert r.spline.values.dtype == np.float32 and np.allclose(r.spline.values, K.Y0, atol=0.05)
