"""Caller-side difference-panel GEMM (workloads_gemm.hip, k_tanh_linear_batched_dma<NK, true, true>): at n = 128 the default entry
wl_tanh_linear_fbd_d forks each 16-point group off the base point's MFMA chain (tlb_fork_*) when X has the finite-difference
structure, and runs the dense GEMM otherwise. wl_tanh_linear_fbd_dense_d always runs the dense GEMM. Both must give the same
bits: on finite-difference points built like k_fd_points, on X that breaks the structure by one ulp, a signed zero or a NaN, and
through whole solves."""
import ctypes as C

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, workloads as W
import problems as P

pytestmark = pytest.mark.gpu


def fd_points(x, lower, upper, eps):
    """X of k_fd_points: rows 2 j, 2 j + 1 are x with coordinate j set to min(x_j + eps, u_j), max(x_j - eps, l_j)."""
    n = x.size
    X = np.repeat(x[None, :], 2 * n, axis=0)
    j = np.arange(n)
    X[2 * j, j] = np.minimum(x + eps, upper)
    X[2 * j + 1, j] = np.maximum(x - eps, lower)
    return X


def mixed_point(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, size=n)     # negative entries, mixed magnitudes
    x[n // 3] = 0.0
    lower, upper = np.full(n, -np.inf), np.full(n, np.inf)
    lower[1::7] = x[1::7]                      # x - eps clamped to x: the minus point equals x
    upper[2::7] = x[2::7]                      # x + eps clamped to x
    lower[5] = upper[5] = x[5]                 # collapsed interval: both points equal x
    return x, lower, upper


def both_panels(m, n, X):
    w = P.tanh_linear(m, n)
    prob = W.TanhLinear(w["A"], w["b"])
    dX = api.DeviceBuffer(np.ascontiguousarray(X))
    out = []
    WL = api.workloads_lib()
    ctx = C.c_void_p(C.addressof(prob.ctx))
    for fn in (WL.wl_tanh_linear_fbd_d, WL.wl_tanh_linear_fbd_dense_d):
        dD = api.DeviceBuffer(np.full((m, n), 7.0))
        fn(ctx, C.c_size_t(m), C.c_size_t(n), C.c_size_t(2 * n), C.c_void_p(dX.ptr), C.c_void_p(dD.ptr))
        prob.stream.synchronize()
        out.append(dD.download())
        dD.free()
    dX.free()
    return w, out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n", [32, 64, 128])
@pytest.mark.parametrize("m", [32, 33, 4097, 40000, 16 * 256 * 3 + 5])
def test_forked_panel_equals_dense_panel_on_fd_points(m, n):
    x, lower, upper = mixed_point(n, 100 * n + m % 97)
    X = fd_points(x, lower, upper, 2.0 ** -20)
    w, (Df, Dd) = both_panels(m, n, X)
    assert same_bits(Df, Dd)
    y = np.tanh(w["A"] @ X.T) - w["b"][:, None]
    assert np.allclose(Df, y[:, 0::2] - y[:, 1::2], rtol=0, atol=1e-12)
    assert np.all(Df[:, 5] == 0.0) and np.abs(Df).max() > 0


# (point, coordinate) pairs at n = 128: the forked chain of point 255 (group 15) takes k-steps 0..29 -- coordinates 0..119 -- from
# the base chain; point 130 (group 8) takes coordinates 0..63; point 0 (group 0) takes none
@pytest.mark.parametrize("kind", ["ulp", "negzero", "nan"])
@pytest.mark.parametrize("where", [(255, 0), (255, 119), (130, 63), (130, 64), (0, 100), (17, 127)])
def test_panel_on_x_without_the_fd_structure_equals_dense(kind, where):
    m, n = 4097, 128
    x, lower, upper = mixed_point(n, 7)
    p, k = where
    if kind == "negzero":
        x[k] = 0.0
    X = fd_points(x, lower, upper, 2.0 ** -20)
    if kind == "ulp":
        X[p, k] = np.nextafter(X[p, k], np.inf)
    elif kind == "negzero":
        X[p, k] = -0.0
    else:
        X[p, k] = np.nan
    _, (Df, Dd) = both_panels(m, n, X)
    assert same_bits(Df, Dd)


@pytest.mark.parametrize("bounded", [False, True])
def test_solve_through_forked_panel_equals_dense_panel_solve(bounded):
    m, n = 50000, 128
    w = P.tanh_linear(m, n)
    lo = up = None
    x0 = w["x0"]
    if bounded:
        lo = np.where(np.arange(n) % 3 == 0, w["xstar"] + 0.02, -np.inf)
        up = np.full(n, np.inf)
        x0 = np.maximum(x0, lo)
    out = []
    for entry in ("wl_tanh_linear_fbd_d", "wl_tanh_linear_fbd_dense_d"):
        prob = W.TanhLinear(w["A"], w["b"])
        prob.fbd = C.cast(getattr(api.workloads_lib(), entry), C.c_void_p).value
        s = M.LeastSquaresSettings(); s.absTolerance = 1e-9
        st = M.Stats()
        res, x = prob.solve(x0, l=lo, u=up, settings=s, batched=True, stats=st)
        assert st.jacobian_full >= 1
        out.append((res, x))
    (rf, xf), (rd, xd) = out
    assert int(rf.status) >= 0 and rf.status == rd.status
    assert np.array_equal(xf, xd) and rf.residual == rd.residual
    assert rf.iterations == rd.iterations and rf.fCalls == rd.fCalls
