"""fitSpline on device-resident points, the part that needs no GPU: the shared arithmetic of csrc/spline_c2.h (its host
instance, mir_fit_spline_eval_host_*) against fit_spline.cpp with array_equal -- both sides are the same sequence of
correctly rounded + - * / sqrt with contraction off, so equality is the expectation, not a tolerance --, the argument codes
mir_fit_spline_gpu_* answers before its first HIP call, and the oracle's status on every fit-level input the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

import fit_spline_cases as K
import mir_optim_amd as M
from mir_optim_amd import api


@pytest.mark.parametrize("nx", [10, 37])
def test_pivoting_knots_pivot(nx):
    """From the factor's pivot record: the pivoting family takes the row-exchange path of the elimination (else that path
    would be untested without anyone noticing). Spacings that only alternate between 0.02 and 1.0 never exchange rows
    (fit_spline_cases.knots says why), which is why there is a third family; the record of that is asserted too."""
    F = M.fit_spline_factor(K.knots(nx, "pivoting"))
    assert set(np.unique(F["swap"])) <= {0.0, 1.0}
    assert F["swap"][:nx - 1].sum() >= 1
    assert F["swap"][nx - 1] == 0                      # there are nx - 1 steps
    assert M.fit_spline_factor(K.knots(nx, "pivoting"), np.float32)["swap"].sum() >= 1
    assert M.fit_spline_factor(K.knots(nx, "alternating"))["swap"].sum() == 0
    assert M.fit_spline_factor(K.knots(nx, "uniform"))["swap"].sum() == 0


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("nx", K.GRID_NX)
def test_shared_arithmetic_equals_fit_spline_cpp(nx, family):
    x, cases = K.grid_cases(nx, family)
    for lam, pts, V in cases:
        p, m = V.shape[0], pts.shape[0] + (1 if lam == 0 else 0)
        ref = K.reference_residuals(pts, x, lam, V)
        got = M.fit_spline_eval_host(pts, x, lam, V, mode=0)
        assert got.shape == (p, m)
        assert np.array_equal(got, ref), (nx, family, lam, pts.shape[0], p, np.abs(got - ref).max())
        D = M.fit_spline_eval_host(pts, x, lam, V, mode=1)
        assert D.size == m * nx + (m if p == 2 * nx + 1 else 0)
        assert np.array_equal(D[:m * nx].reshape(m, nx), (ref[0:2 * nx:2] - ref[1:2 * nx:2]).T), (nx, family, lam, pts.shape[0], p)
        if p == 2 * nx + 1:
            assert np.array_equal(D[m * nx:], ref[2 * nx])


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("nx", K.GRID_NX)
def test_shared_arithmetic_float_equals_float_run_of_fit_spline_cpp(nx, family):
    """Float: mode 0 (the one the float entry uses) on four of each case's vectors against a float run of fit_spline.cpp's own
    functions; mode 1 against the differences of mode 0."""
    x, cases = K.grid_cases(nx, family)
    x32 = x.astype(np.float32)
    if np.any(np.diff(x32) <= 0):
        pytest.fail("knots collapse in float")
    for lam, pts, V in cases:
        p, m = V.shape[0], pts.shape[0] + (1 if lam == 0 else 0)
        got = M.fit_spline_eval_host(pts, x, lam, V, mode=0, dtype=np.float32)
        pick = sorted({0, 1, p // 2, p - 1})
        ref = K.reference_residuals_f32(pts, x, lam, V[pick])
        assert got.dtype == np.float32 and np.array_equal(got[pick], ref), (nx, family, lam, pts.shape[0], p)
        D = M.fit_spline_eval_host(pts, x, lam, V, mode=1, dtype=np.float32)
        assert np.array_equal(D[:m * nx].reshape(m, nx), (got[0:2 * nx:2] - got[1:2 * nx:2]).T)
        if p == 2 * nx + 1:
            assert np.array_equal(D[m * nx:], got[2 * nx])


@pytest.mark.parametrize("suf,ct,S,R", [("d", np.float64, api._Sd, api._Rd), ("s", np.float32, api._Ss, api._Rs)])
def test_argument_codes_come_before_any_device_call(suf, ct, S, R):
    """Every code below is answered from the arguments alone: `points` is an address that is never dereferenced."""
    fn = getattr(M.lib(), "mir_fit_spline_gpu_" + suf)
    OK, FEW, BAD = 0, 1, 2
    nx = 10
    x = K.X.astype(ct)
    lo, up = np.full(nx, -np.inf, dtype=ct), np.full(nx, np.inf, dtype=ct)
    y, d = np.zeros(nx, dtype=ct), np.zeros(nx, dtype=ct)
    raw = R()
    fake = 0x1000                                       # stands for a device pointer

    def call(npoints=10, points=fake, nx_=nx, x_=x.ctypes.data, l_=lo.ctypes.data, u_=up.ctypes.data, lam=1e-3, opt=None,
             y_=y.ctypes.data, res=C.byref(raw)):
        return fn(None, npoints, points, nx_, x_, l_, u_, lam, C.byref(opt) if opt is not None else None, y_, d.ctypes.data, res)

    assert call(points=None) == BAD and call(x_=None) == BAD and call(l_=None) == BAD and call(u_=None) == BAD
    assert call(y_=None) == BAD and call(res=None) == BAD
    assert call(nx_=0) == BAD
    assert call(lam=-1.0) == BAD and call(lam=float("nan")) == BAD
    assert call(npoints=0) == BAD and call(npoints=0, lam=0.0) == BAD
    keep = C.c_int(0)
    addr = C.addressof(keep)
    for field in ("comm", "fb", "fbContext", "fbRowMajor", "fbRowMajorDiff"):
        assert call(opt=M.GpuOptions(**{field: addr})) == BAD, field
    assert call(npoints=9, lam=0.0) == FEW                # FS:47-51
    assert call(npoints=9, lam=0.0, opt=M.GpuOptions(fb=addr)) == BAD   # bad arguments are reported first, as in mir_fit_spline_*
    assert FEW != OK
    with pytest.raises(ValueError):
        M.fitSplineGpu(None, K.POINTS, K.X, lo, up, -1.0)
    with pytest.raises(Exception, match="greater or equal"):
        M.fitSplineGpu(None, K.POINTS[:5], K.X, lo, up, 0.0)


def test_eval_entries_check_their_arguments():
    L = M.lib()
    one = np.ones(4)
    assert L.mir_fit_spline_eval_host_d(0, one.ctypes.data, 2, one.ctypes.data, 0.0, 1, one.ctypes.data, 0, one.ctypes.data) == -1
    assert L.mir_fit_spline_eval_host_d(2, one.ctypes.data, 2, one.ctypes.data, 0.0, 3, one.ctypes.data, 1, one.ctypes.data) == -1
    assert L.mir_fit_spline_gpu_eval_d(2, None, 2, one.ctypes.data, 0.0, 1, one.ctypes.data, 0, one.ctypes.data) == -1
    assert L.mir_fit_spline_gpu_eval_s(2, 0x1000, 2, one.ctypes.data, 0.0, 4, one.ctypes.data, 1, one.ctypes.data) == -1   # mode 1 is f64
    assert L.mir_spline_eval_gpu_d(0, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0x1000, 0x1000, None) == -1
    assert L.mir_spline_eval_gpu_d(2, one.ctypes.data, one.ctypes.data, one.ctypes.data, 0, None, None, None) == 0
    assert L.mir_fit_spline_factor_d(0, one.ctypes.data, one.ctypes.data) == -1


@pytest.mark.parametrize("case", K.fit_cases(), ids=lambda c: c[0])
def test_oracle_converges_on_the_fit_level_inputs(oracle, case):
    """The GPU comparisons skip no case, so every input has to end inside the default maxIterations in the oracle."""
    name, pts, x, lam, lo, up = case

    def f(v, y):
        y[:] = M.fit_spline_residuals(pts, x, lam, v)
    bounded = np.any(np.isfinite(lo))
    kw = dict(lower=lo, upper=up) if bounded else {}
    res, v = oracle.optimize(f, pts.shape[0] + (1 if lam == 0 else 0), np.zeros(x.size), **kw)
    assert res.status >= 0, (name, res.status, res.iterations)
    assert np.all(np.isfinite(v))
