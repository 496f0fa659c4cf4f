"""Problem families of the 9 to 16 parameter batched fit, shared by tests/test_gpu_batched16.py and scripts/batched16.py (not a
test module). The harmonic family: t = linspace(0, 4, m); p0 exp(-t p1) + p2 + sum_j p_j h_j(t) with h_j = sin / cos(k pi / 2 t)
for odd / even j, k = (j - 1) // 2; truth, start and noise of problem k from splitmix64_uniform(700 + k, m + 2 n). The
three-Gaussian family of MODEL16_GAUSS3_AFFINE by the same seeds. pad8_problems: cfg 5's n = 8 family in float64 (the seeds
and formulas of problems.cfg5_pad8), for scale in the measurement script."""
import functools

import numpy as np

import problems as P

RDT = np.dtype([("status", "<i4"), ("iterations", "<u4"), ("fCalls", "<u4"), ("gCalls", "<u4"), ("residual", "<f8"),
                ("lambda", "<f8")])          # mir_least_squares_result_d
COUNT = 64


def harm_basis(n, t):
    """rows j = 3 .. n - 1 of the harmonic terms"""
    w = np.pi / 2
    return np.stack([np.sin((j - 1) // 2 * w * t) if j % 2 else np.cos((j - 1) // 2 * w * t) for j in range(3, n)])


def harm_value(B, t, p):
    return p[0] * np.exp(-t * p[1]) + p[2] + p[3:] @ B


@functools.lru_cache(maxsize=None)
def harm_problems(n, m, count=COUNT):
    t = np.linspace(0.0, 4.0, m)
    B = harm_basis(n, t)
    data = np.empty((count, m)); truth = np.empty((count, n)); x0 = np.empty((count, n))
    for k in range(count):
        u = P.splitmix64_uniform(700 + k, m + 2 * n)
        p = np.concatenate([[1.0 + u[0], 1.5 + 2.0 * u[1], 0.2 * u[2]], 0.6 * u[3:n] - 0.3])
        truth[k] = p
        data[k] = harm_value(B, t, p) + 0.01 * (2 * u[2 * n:] - 1)
        x0[k] = p
        x0[k, :2] *= 1 + 0.2 * (2 * u[n:n + 2] - 1)
        x0[k, 2:] += 0.1 * (2 * u[n + 2:2 * n] - 1)
    for a in (t, B, data, truth, x0):
        a.setflags(write=False)
    return t, B, data, truth, x0


def gauss3_value(t, p):
    v = p[9] + p[10] * t
    for k in range(3):
        v = v + p[3 * k] * np.exp(-0.5 * ((t - p[3 * k + 1]) / p[3 * k + 2]) ** 2)
    return v


@functools.lru_cache(maxsize=None)
def gauss3_problems(m=130, count=COUNT):
    t = np.linspace(0.0, 4.0, m)
    n = 11
    data = np.empty((count, m)); x0 = np.empty((count, n))
    for k in range(count):
        u = P.splitmix64_uniform(700 + k, m + 2 * n)
        p = np.array([1 + u[0], 0.8 + 0.2 * u[1], 0.15 + 0.1 * u[2], 1 + u[3], 2.0 + 0.2 * u[4], 0.15 + 0.1 * u[5],
                      1 + u[6], 3.1 + 0.2 * u[7], 0.15 + 0.1 * u[8], 0.2 * u[9], 0.1 * u[10] - 0.05])
        data[k] = gauss3_value(t, p) + 0.01 * (2 * u[2 * n:] - 1)
        x0[k] = p * (1 + 0.1 * (2 * u[n:2 * n] - 1))
    for a in (t, data, x0):
        a.setflags(write=False)
    return t, data, x0


def pad8_problems(count, m=512, noise=0.01):
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 8))
    basis = np.stack([np.sin(2 * t), np.cos(2 * t), np.sin(5 * t), np.cos(5 * t), t])
    for k in range(count):
        u = P.splitmix64_uniform(100 + k, m + 16)
        p = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2], 0.6 * u[3] - 0.3, 0.6 * u[4] - 0.3, 0.6 * u[5] - 0.3,
                      0.6 * u[6] - 0.3, 0.1 * u[7] - 0.05])
        data[k] = p[0] * np.exp(-t * p[1]) + p[2] + p[3:] @ basis + noise * (2 * u[16:] - 1)
        x0[k] = p
        x0[k, :2] *= 1 + 0.2 * (2 * u[8:10] - 1)
        x0[k, 2:] += 0.1 * (2 * u[10:16] - 1)
    return t, data, x0
