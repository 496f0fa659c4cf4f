"""A caller's own DOUBLE model on the batched one-wavefront-per-problem path: tests/user_model/user_model_f64.hip declares
`using value_type = double;`, five parameters and its own derivative, and is compiled against include/mir_optim_amd_batched.hpp
into a library of its own. Every problem against the oracle's double instantiation minimising the same expression in numpy --
with finite differences, and with MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN against the oracle given the same analytic Jacobian (g):
same status class, residual to rtol 1e-9 and x to rtol 1e-6 on at least 95 % of the problems, the rest within 1e-7 / 1e-3
(tests/test_gpu_batched_f64.py says why iteration counts are not compared); with the analytic Jacobian, gCalls counts the
refreshes and the fit needs fewer residual evaluations than with finite differences."""
import ctypes as C

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import problems as P

pytestmark = pytest.mark.gpu

N = 5
RDT = np.dtype([("status", "<i4"), ("iterations", "<u4"), ("fCalls", "<u4"), ("gCalls", "<u4"), ("residual", "<f8"),
                ("lambda", "<f8")])


def model(t, x):
    """the expression of DampedCosineD"""
    return x[0] * np.exp(-x[1] * t) * np.cos(x[2] * t) + x[3] + x[4] * np.sqrt(t)


def model_grad(t, x):
    e = np.exp(-x[1] * t); c = np.cos(x[2] * t); s_ = np.sin(x[2] * t)
    return np.stack([e * c, -t * x[0] * e * c, -t * x[0] * e * s_, np.ones_like(t), np.sqrt(t)], axis=1)


def make(count, m, noise=0.01):
    t = np.linspace(0.05, 6.0, m)
    data = np.empty((count, m)); truth = np.empty((count, N)); x0 = np.empty((count, N))
    for k in range(count):
        u = P.splitmix64_uniform(900 + k, m + 16)
        p = np.array([1.0 + u[0], 0.2 + 0.6 * u[1], 2.0 + 2.0 * u[2], 0.4 * u[4] - 0.2, 0.2 * u[5] - 0.1])
        truth[k] = p
        data[k] = model(t, p) + noise * (2 * u[16:] - 1)
        x0[k] = p * (1 + 0.08 * (2 * u[8:8 + N] - 1)) + 0.02 * (2 * u[8:8 + N] - 1)
    return t, data, truth, x0


def test_user_f64_model_with_finite_differences_and_with_its_own_gradient(oracle):
    count, m = 64, 384
    t, data, truth, x0 = make(count, m)
    UL = C.CDLL(hipbuild.user_model_f64_lib())
    UL.user_fit_damped_cosine_d.restype = C.c_int
    UL.user_fit_damped_cosine_d.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    s = M.LeastSquaresSettings(np.float64)
    lo = np.full(N, -np.inf); up = np.full(N, np.inf)
    dt_, dd, dx = api.DeviceBuffer(t), api.DeviceBuffer(data), api.DeviceBuffer(x0)
    dlo, dup = api.DeviceBuffer(lo), api.DeviceBuffer(up)
    dres = api.DeviceBuffer(nbytes=count * 32, dtype=np.uint8, shape=(count * 32,))
    st = api.Stream()
    outs = {}
    for variant in (2, 0):                                 # MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN, finite differences
        dx.upload(x0)
        opt = api.BatchedOptions(stream=st.handle, variant=variant)
        assert UL.user_fit_damped_cosine_d(C.addressof(s), count, m, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, 0, dd.ptr, dres.ptr,
                                           C.addressof(opt)) == 0
        st.synchronize()
        outs[variant] = (np.frombuffer(dres.download().tobytes(), dtype=RDT).copy(), dx.download().reshape(count, N).copy())
    for b in (dt_, dd, dx, dlo, dup, dres):
        b.free()
    raw_g, x_g = outs[2]
    raw_fd, x_fd = outs[0]
    assert (raw_g["status"] >= 0).all() and (raw_fd["status"] >= 0).all()
    assert (raw_g["gCalls"] >= 1).all() and (raw_fd["gCalls"] == 0).all()
    assert raw_g["fCalls"].sum() < raw_fd["fCalls"].sum()
    so = oracle.default_settings(np.float64)
    for raw, x, use_g in ((raw_g, x_g, True), (raw_fd, x_fd, False)):
        loose = []
        for k in range(count):
            d = data[k]

            def f(xv, y, d=d):
                y[:] = model(t, np.asarray(xv)) - d

            def g(xv, J):
                J[:, :] = model_grad(t, np.asarray(xv))
            ro, xo = oracle.optimize(f, m, x0[k], g=g if use_g else None, settings=so, dtype=np.float64)
            assert ro.status >= 0, (k, ro.status)
            rgap = abs(raw["residual"][k] / ro.residual - 1)
            assert rgap <= 1e-7, (k, use_g, raw["residual"][k], ro.residual)
            if use_g:
                # the reference's g path on both sides: refreshes are counted in gCalls, with an age limit of 3 (LS:945) --
                # a g refresh at most every fourth accepted step, so fewer residual evaluations than finite differences
                assert ro.gCalls >= 1 and raw["gCalls"][k] >= (raw["iterations"][k] + 3) // 4, (k, raw["gCalls"][k], raw["iterations"][k])
            if not (np.allclose(x[k], xo, rtol=1e-6, atol=1e-7) and rgap <= 1e-9):
                loose.append((k, float(np.max(np.abs(x[k] - xo) / np.maximum(np.abs(xo), 1e-3)))))
                assert np.allclose(x[k], xo, rtol=1e-3, atol=1e-4), (k, use_g, x[k], xo)
        assert len(loose) <= 0.05 * count, (use_g, loose)
