"""Covariance of the fitted parameters of the general solver (mir_lsq_covariance_gpu_* / M.covariance) against numpy.

Problem: tests/problems.py::tanh_linear, r_i(x) = tanh(a_i . x) - b_i. Reference in float64: J_ij = (1 - tanh^2(a_i . x)) a_ij,
cov_ref = ||r||^2 / (m - n) inv(J^T J). The figure compared is the largest |cov - cov_ref|_ij / (sd_i sd_j) with
sd = sqrt(diag(cov_ref)).

cond(J^T J) of the reference (numpy, CPU): 2000 x 8: 1.74; 4096 x 128: 3.15; 1500 x 300: 7.82 -- the
rows of tanh_linear are scaled by sqrt(3 / n), numpy's own inverse is good to ~cond x 1e-16, far below every tolerance here.

Measured on an MI355X (profiles/r09/covariance.txt):
    f64, analytic g, host callbacks 2000 x 8                8.939e-16
    f64, finite differences                                 1.321e-08   (host callbacks 2000 x 8: 2.973e-10; device callbacks
                                                                         4096 x 128: 4.050e-09, 1500 x 300: 1.321e-08)
    f32, finite differences, host callbacks 2000 x 8        1.540e-05
The tolerances are 8 x these values. The batched analogue measured 3e-14, 6e-9 .. 1.3e-7 and 1e-4 .. 3e-2:
every figure here is below its counterpart.

Device-callback variants (fb only / fbRowMajor / fbRowMajorDiff) and their bits, as a solve's refreshes have them
(tests/test_gpu_fd_fused.py): at n = 128 the pair panel and the difference panel run the same stage partition and agree to the
bit, the point-major path (k_fd_fill + the plain J^T J kernel) agrees to rounding; at n = 300 no fused kernel covers the shape,
all three take the point-major path and agree to the bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api
from mir_optim_amd import parallel as PAR
from mir_optim_amd import workloads as W
import problems as P

pytestmark = pytest.mark.gpu

TOL_G64 = 8 * 8.939e-16
TOL_FD64 = 8 * 1.321e-08
TOL_FD32 = 8 * 1.540e-05
# A parameter on its upper bound: the difference is one-sided over h = jacobianEpsilon = 2^-26. Its truncation error relative to
# the column is h/2 |tanh''/tanh'| |a_ij| = h |tanh| |a_ij| <= 1.5e-8 x 1 x sqrt(3/8) = 9.1e-9; a relative error e of one column
# of J changes the normalised covariance by at most 2 cond(J^T J) e = 2 x 1.74 x 9.1e-9 = 3.2e-8; the rounding part is the
# finite-difference tolerance (the interval is h instead of 2 h: twice the central difference's 2.973e-10, far inside it)
TOL_ONE_SIDED = 3.2e-8 + TOL_FD64
# sharded against unsharded: J^T J is summed in another order, relative error <= m eps (2001 x 1.1e-16 = 2e-13) in the worst
# case, amplified by cond(J^T J) (< 10): 2e-12; the bound leaves a factor of five
TOL_SHARDED = 1e-11


def reference(w, x, free=None):
    """(cov_ref, sd, ||r||^2) in float64; free: indices kept (the reduced problem)"""
    A, b = w["A"], w["b"]
    t = np.tanh(A @ x)
    r = t - b
    J = (1 - t * t)[:, None] * A
    if free is not None:
        J = J[:, free]
    m, n = J.shape
    cov = (r @ r) / (m - n) * np.linalg.inv(J.T @ J)
    return cov, np.sqrt(np.diag(cov)), r @ r


def deviation(cov, cov_ref, sd):
    return np.abs((np.asarray(cov, dtype=np.float64) - cov_ref) / np.outer(sd, sd)).max()


@functools.lru_cache(maxsize=None)
def small():
    """2000 x 8 at the known minimiser's neighbourhood: host callbacks, reference computed once"""
    w = P.tanh_linear(2000, 8)
    x = w["xstar"].copy()
    return w, x, reference(w, x)


def host_f(w, dtype):
    A, b = w["A"].astype(dtype), w["b"].astype(dtype)

    def f(x, y):
        y[:] = np.tanh(A @ x) - b
    return f


def host_g(w):
    A = w["A"]

    def g(x, J):
        t = np.tanh(A @ x)
        J[:] = (1 - t * t)[:, None] * A
    return g


def test_host_callbacks_with_analytic_jacobian():
    w, x, (cr, sd, rr) = small()
    x_in = x.copy()
    cov, stderr, res, info = M.covariance(host_f(w, np.float64), 2000, x_in, g=host_g(w))
    d = deviation(cov, cr, sd)
    print(f"covariance f64 g 2000x8: deviation {d:.3e}")
    assert info == 0 and np.array_equal(x_in, x) and np.array_equal(cov, cov.T)
    assert np.isclose(res, rr, rtol=1e-12) and np.allclose(stderr, np.sqrt(np.diag(cov)), rtol=0, atol=0)
    assert d <= TOL_G64


@pytest.mark.parametrize("dtype,tol", [(np.float64, TOL_FD64), (np.float32, TOL_FD32)])
def test_host_callbacks_with_finite_differences(dtype, tol):
    w, x, (cr, sd, rr) = small()
    cov, stderr, res, info = M.covariance(host_f(w, dtype), 2000, x, dtype=dtype)
    d = deviation(cov, cr, sd)
    print(f"covariance {np.dtype(dtype).name} fd host 2000x8: deviation {d:.3e}")
    assert info == 0 and cov.dtype == dtype and np.array_equal(cov, cov.T)
    assert np.isclose(res, rr, rtol=1e-12 if dtype == np.float64 else 1e-4)
    assert d <= tol


def test_absolute_sigma_fixed_parameter_and_no_degrees_of_freedom():
    w, x, (cr, sd, rr) = small()
    f, g = host_f(w, np.float64), host_g(w)
    cov, _, res, _ = M.covariance(f, 2000, x, g=g)
    cov_abs, _, _, _ = M.covariance(f, 2000, x, g=g, absolute_sigma=True)
    s2 = res / (2000 - 8)
    assert np.allclose(cov_abs, cov / s2, rtol=4e-16 * 4, atol=0)      # one multiplication and one division apart
    # one parameter fixed by l == u: its row and column are 0, the rest is the reduced problem with dof = m - (n - 1)
    lo, up = np.full(8, -np.inf), np.full(8, np.inf)
    lo[3] = up[3] = x[3]
    free = np.array([0, 1, 2, 4, 5, 6, 7])
    for gg, tol in ((g, TOL_G64), (None, TOL_FD64)):
        cf, se, _, info = M.covariance(f, 2000, x, lo, up, g=gg)
        crf, sdf, _ = reference(w, x, free)
        df = deviation(cf[np.ix_(free, free)], crf, sdf)
        print(f"covariance f64 {'g' if gg else 'fd'} host 2000x8, parameter 3 fixed: deviation {df:.3e}")
        assert info == 0 and np.all(cf[3] == 0) and np.all(cf[:, 3] == 0) and se[3] == 0
        assert df <= tol
    # a parameter ON a bound with l < u is not fixed: a one-sided difference, a variance like any other
    lo2, up2 = np.full(8, -np.inf), np.full(8, np.inf)
    up2[3] = x[3]
    cb, _, _, info = M.covariance(f, 2000, x, lo2, up2)
    d1 = deviation(cb, cr, sd)
    print(f"covariance f64 fd host 2000x8, parameter 3 on its upper bound (one-sided difference): deviation {d1:.3e}")
    assert info == 0 and cb[3, 3] > 0 and d1 <= TOL_ONE_SIDED
    # m = n: no degrees of freedom
    w8 = P.tanh_linear(8, 8)
    c8, se8, _, info = M.covariance(host_f(w8, np.float64), 8, w8["xstar"], g=host_g(w8))
    assert info == 0 and np.all(np.isposinf(c8)) and np.all(np.isposinf(se8))
    c8a, _, _, _ = M.covariance(host_f(w8, np.float64), 8, w8["xstar"], g=host_g(w8), absolute_sigma=True)
    assert np.all(np.isfinite(c8a))


def dev_cov(prob, x, mode, workspace=None, stats=None, **kw):
    opts = prob.options(batched=mode, workspace=workspace, stats=stats)
    return M.covariance(prob.f, prob.m, x, options=opts, fContext=C.addressof(prob.ctx), **kw)


@pytest.mark.parametrize("m,n", [(4096, 128), (1500, 300)])
def test_device_callbacks_three_panels_and_the_workspace(m, n):
    w = P.tanh_linear(m, n)
    prob = W.TanhLinear(w["A"], w["b"])
    ws = api.lib().mir_lsq_workspace_create(m, n, 8)
    assert ws
    try:
        s = M.LeastSquaresSettings(); s.absTolerance = 1e-9
        r1, x1 = prob.solve(w["x0"], settings=s, batched=True, workspace=ws)
        assert r1.status >= 0
        x = x1.copy()
        cr, sd, rr = reference(w, x)
        out = {}
        for mode in ("pointmajor", "rowmajor", True):
            st = M.Stats()
            cov, se, res, info = dev_cov(prob, x, mode, stats=st)
            d = deviation(cov, cr, sd)
            print(f"covariance f64 fd device {m}x{n} {mode}: deviation {d:.3e}")
            assert info == 0 and np.array_equal(x, x1) and np.array_equal(cov, cov.T) and np.isclose(res, rr, rtol=1e-12)
            assert d <= TOL_FD64
            assert st.jacobian_full == 1 and st.jacobian_broyden == 0 and st.fd_callback_points == 2 * n and st.solve_launches == 0
            out[mode] = cov
        if n == 128:
            assert np.array_equal(out["rowmajor"], out[True])            # pair panel == difference panel (n % 64 == 0)
            assert deviation(out["pointmajor"], out[True], sd) <= TOL_FD64
        else:
            assert np.array_equal(out["pointmajor"], out["rowmajor"]) and np.array_equal(out["rowmajor"], out[True])
        # with the solve's workspace: the bits of a call without one; the workspace then serves a second solve unchanged
        cw, _, _, info = dev_cov(prob, x, True, workspace=ws)
        assert info == 0 and np.array_equal(cw, out[True])
        r2, x2 = prob.solve(w["x0"], settings=s, batched=True, workspace=ws)
        assert np.array_equal(x2, x1) and r2.residual == r1.residual and r2.iterations == r1.iterations and r2.status == r1.status
    finally:
        api.lib().mir_lsq_workspace_destroy(ws)


def test_two_rank_group_gives_every_rank_the_unsharded_covariance():
    import threading
    m_total, n, world = 2001, 8, 2
    w = P.tanh_linear(m_total, n)
    x = w["xstar"].copy()
    cr, sd, _ = reference(w, x)
    whole = W.TanhLinear(w["A"], w["b"])
    c1, _, res1, _ = dev_cov(whole, x, True)
    comms, close = PAR.local_group(world)
    probs = []
    for r in range(world):
        off, ml = PAR.row_shard(m_total, world, r)
        ws = P.tanh_linear(ml, n, row_offset=off)
        probs.append(W.TanhLinear(ws["A"], ws["b"]))
    out, errs = [None] * world, [None] * world

    def one(r):
        try:
            opts = probs[r].options(batched=True, comm=comms[r])
            out[r] = M.covariance(probs[r].f, probs[r].m, x, options=opts, fContext=C.addressof(probs[r].ctx))
        except BaseException as e:     # noqa: BLE001 -- reported in the main thread
            errs[r] = e
    ts = [threading.Thread(target=one, args=(r,)) for r in range(world)]
    try:
        for t in ts:
            t.start()
        for t in ts:
            t.join(300)
        assert not any(t.is_alive() for t in ts), "a shard thread hangs"
    finally:
        close()
    for e in errs:
        if e is not None:
            raise e
    for r in range(world):
        cov, _, res, info = out[r]
        d = deviation(cov, c1, sd)
        print(f"covariance sharded rank {r}: deviation from the unsharded call {d:.3e}")
        assert info == 0 and d <= TOL_SHARDED and np.isclose(res, res1, rtol=1e-13)     # s^2 with the TOTAL row count
        assert deviation(cov, cr, sd) <= TOL_FD64
    assert np.array_equal(out[0][0], out[1][0])                          # the sum runs in rank order: the same bits on every rank
