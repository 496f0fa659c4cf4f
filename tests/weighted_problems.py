"""Problem sets and the numpy reference of the weighted batched fits (tests/test_batched_weighted_host.py,
tests/test_gpu_batched_weighted.py): heteroscedastic data with weights w = 1 / sigma, every fourth problem with its last 37
rows at weight 0, and the float64 covariance s^2 inv(J^T J) from the analytic model Jacobian."""
import numpy as np

import problems as P

ZERO_TAIL = 37
EXP_DECAY, EXP3_AFFINE, PAD8 = 0, 1, 2          # MIR_LSQ_MODEL_*


def model_value(model, t, p):
    if model == EXP_DECAY:
        return p[0] * np.exp(-t * p[1]) + p[2]
    if model == EXP3_AFFINE:
        return p[0] * np.exp(-t * p[1]) + p[2] * np.exp(-t * p[3]) + p[4] * np.exp(-t * p[5]) + p[6] + p[7] * t
    return (p[0] * np.exp(-t * p[1]) + p[2] + p[3] * np.sin(2 * t) + p[4] * np.cos(2 * t) + p[5] * np.sin(5 * t)
            + p[6] * np.cos(5 * t) + p[7] * t)


def model_jacobian(model, t, p):
    """d model / d p, m x n, float64"""
    t = np.asarray(t, dtype=np.float64); p = np.asarray(p, dtype=np.float64)
    e = np.exp(-t * p[1])
    one = np.ones_like(t)
    if model == EXP_DECAY:
        return np.stack([e, -t * p[0] * e, one], axis=1)
    if model == EXP3_AFFINE:
        cols = []
        for k in range(3):
            ek = np.exp(-t * p[2 * k + 1])
            cols += [ek, -t * p[2 * k] * ek]
        return np.stack(cols + [one, t], axis=1)
    return np.stack([e, -t * p[0] * e, one, np.sin(2 * t), np.cos(2 * t), np.sin(5 * t), np.cos(5 * t), t], axis=1)


def _sigma(clean):
    return 0.01 * np.sqrt(np.abs(clean) / np.max(np.abs(clean))) + 0.002


def exp_decay_weighted(count, m=512):
    """m = 512, t = linspace(0, 4); problem k from splitmix64_uniform(900 + k, 2 m + 6): truth [1 + u0, 0.5 + 2 u1, 0.2 u2],
    start = truth (1 + 0.3 (2 u[3:6] - 1)), sigma_i = 0.01 sqrt(clean_i / max clean) + 0.002, w = 1 / sigma,
    data = clean + 1.7 sigma (2 u[6:6 + m] - 1); every fourth problem has its last 37 weights set to 0. float64."""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 3)); w = np.empty((count, m))
    for k in range(count):
        u = P.splitmix64_uniform(900 + k, 2 * m + 6)
        truth = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2]])
        x0[k] = truth * (1 + 0.3 * (2 * u[3:6] - 1))
        clean = model_value(EXP_DECAY, t, truth)
        sigma = _sigma(clean)
        w[k] = 1.0 / sigma
        data[k] = clean + 1.7 * sigma * (2 * u[6:6 + m] - 1)
        if k % 4 == 0:
            w[k, m - ZERO_TAIL:] = 0.0
    return t, data, x0, w


def pad8_weighted(count, m=512):
    """the same recipe on the n = 8 family of cfg 5 (tests/problems.py cfg5_pad8: truth and start as there, seeds 900 + k)"""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 8)); w = np.empty((count, m))
    for k in range(count):
        u = P.splitmix64_uniform(900 + k, 2 * m + 16)
        p = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2], 0.6 * u[3] - 0.3, 0.6 * u[4] - 0.3, 0.6 * u[5] - 0.3,
                      0.6 * u[6] - 0.3, 0.1 * u[7] - 0.05])
        x0[k] = p
        x0[k, :2] *= 1 + 0.2 * (2 * u[8:10] - 1)
        x0[k, 2:] += 0.1 * (2 * u[10:16] - 1)
        clean = model_value(PAD8, t, p)
        sigma = _sigma(clean)
        w[k] = 1.0 / sigma
        data[k] = clean + 1.7 * sigma * (2 * u[16:16 + m] - 1)
        if k % 4 == 0:
            w[k, m - ZERO_TAIL:] = 0.0
    return t, data, x0, w


MAKERS = {EXP_DECAY: exp_decay_weighted, PAD8: pad8_weighted}


def weighted_f(model, t, d, w, dtype=np.float64):
    """the reference's residual callback for the weighted objective: y = w (model - d), evaluated in `dtype`"""
    t = np.asarray(t, dtype=dtype); d = np.asarray(d, dtype=dtype); w = np.asarray(w, dtype=dtype)

    def f(p, y):
        y[:] = w * (model_value(model, t, np.asarray(p, dtype=dtype)) - d)
    return f


def reference_covariance(J, w, residual, absolute_sigma=False):
    """float64: inv(J^T J) residual / (rows with nonzero weight - n), J the UNWEIGHTED m x n model Jacobian"""
    J = np.asarray(J, dtype=np.float64) * np.asarray(w, dtype=np.float64)[:, None]
    inv = np.linalg.inv(J.T @ J)
    if absolute_sigma:
        return inv
    dof = int(np.count_nonzero(w)) - J.shape[1]
    return inv * (float(residual) / dof)


def scaled_gap(cov, ref):
    """max_ij |cov_ij - ref_ij| / (sd_i sd_j), sd from the reference"""
    sd = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(np.asarray(cov, dtype=np.float64) - ref) / np.outer(sd, sd)))
