"""Inputs, the numpy float64 reference and the error measures of the fitted-curve / confidence-band tests
(tests/test_batched_predict_host.py, tests/test_gpu_batched_predict.py, scripts/batched_predict.py; not a test module).

The kernel takes x and C as inputs, so a case hands it inputs of its own: x is a problem set's starting points, C is
weighted_problems.reference_covariance at that x (the analytic float64 Jacobian on the set's own t, weights and data), cast to
the dtype. The reference is numpy float64 at the ROUNDED inputs (x, C, tq as the device sees them):
    value   model(tq; x)                                  gap: |v - v_ref| / max(|v_ref|, 1e-3 max_i |v_ref,i|)
    sigma   sqrt(g^T C g), g the analytic gradient        gap: |s - s_ref| / sqrt(sum_j g_j^2 C_jj)   (the uncancelled magnitude:
                                                          the band itself cancels up to 120-fold on the eight-parameter family)
over the free parameters; a parameter whose difference is one-sided in the box takes that one-sided float64 difference as g_j.
cpu_figures() restates the kernel's arithmetic in numpy in the WORKING precision (value; central differences at the settings'
jacobianEpsilon or the analytic gradient; the quadratic form) and measures it the same way: CPU_FIGURE below holds what it gave,
and the bars of the GPU test are 10 x the larger of that and the device's measured worst gap, rounded up to one digit."""
import functools

import numpy as np

import problems as P
import weighted_problems as WP
import batched16_weighted_problems as WP16
from batched16_problems import gauss3_value, harm_basis, harm_value
from test_gpu_batched_weighted import make_peaks, peak_jacobian, peak_value

COUNT = 8
QS = [1, 63, 64, 65, 129]
EPS = {np.float32: 2.0 ** -11, np.float64: 2.0 ** -26}          # jacobianEpsilon of the default settings (the host test holds it)


def grid(q, dtype=np.float64):
    return np.linspace(-0.25, 4.25, q).astype(dtype)


def exp3_weighted(count, m=512):
    """an EXP3_AFFINE set by the recipe of weighted_problems (seeds 1700 + k): three decays with rates near 0.6, 3 and 15 on
    an affine baseline (cond(C) ~ 1e7: the float casts stay positive definite, min_eig_ratio). x0 = the truth moved by up to 5 %."""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 8)); w = np.empty((count, m))
    for k in range(count):
        u = P.splitmix64_uniform(1700 + k, 2 * m + 16)
        p = np.array([1.0 + u[0], 0.5 + 0.2 * u[1], 1.0 + u[2], 2.5 + u[3], 1.0 + u[4], 12.0 + 6.0 * u[5], 0.2 * u[6],
                      0.1 * u[7] - 0.05])
        x0[k] = p * (1 + 0.05 * (2 * u[8:16] - 1))
        clean = WP.model_value(WP.EXP3_AFFINE, t, p)
        sigma = WP._sigma(clean)
        w[k] = 1.0 / sigma
        data[k] = clean + 1.7 * sigma * (2 * u[16:16 + m] - 1)
    return t, data, x0, w


class Family:
    """a model with its numpy value(t, p) / jacobian(t, p) (q x n), and the inputs of its cases: x (COUNT x n) and C (COUNT x n x n)"""

    def __init__(self, name, n, value, jacobian, x, t, data, w):
        self.name, self.n, self.value, self.jacobian = name, n, value, jacobian
        self.x = np.array(x[:COUNT], dtype=np.float64)
        C = []
        for k in range(COUNT):
            r = w[k] * (value(t, self.x[k]) - data[k])
            C.append(WP.reference_covariance(jacobian(t, self.x[k]), w[k], r @ r))
        self.C = np.array(C)
        for a in (self.x, self.C):
            a.setflags(write=False)


def _harm(n):
    value = lambda t, p: harm_value(harm_basis(n, t).astype(t.dtype), t, p)          # noqa: E731
    jac = lambda t, p: WP16.harm_jacobian(harm_basis(n, t), t, p)                      # noqa: E731
    t, B, data, x0, w = WP16.harm_weighted(n, 131)
    return Family("harm%d" % n, n, value, jac, x0, t, data, w)


@functools.lru_cache(maxsize=None)
def family(name):
    if name in ("exp_decay", "pad8", "exp3"):
        model = {"exp_decay": WP.EXP_DECAY, "pad8": WP.PAD8, "exp3": WP.EXP3_AFFINE}[name]
        t, data, x0, w = {"exp_decay": WP.exp_decay_weighted, "pad8": WP.pad8_weighted, "exp3": exp3_weighted}[name](COUNT, 512)
        return Family(name, x0.shape[1], lambda tt, p: WP.model_value(model, tt, p), lambda tt, p: WP.model_jacobian(model, tt, p),
                      x0, t, data, w)
    if name.startswith("harm"):
        return _harm(int(name[4:]))
    if name == "gauss3":
        t, data, x0, w = WP16.gauss3_weighted(130)
        return Family(name, 11, gauss3_value, WP16.gauss3_jacobian, x0, t, data, w)
    assert name == "peak", name
    t, data, x0, w = make_peaks(COUNT, 512)
    return Family(name, 5, peak_value, peak_jacobian, x0, t, data, w)


def box_of(lo, up, k, n):
    """problem k's (lo, up) rows of a box given as None, n values or count x n"""
    lo = np.full(n, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    up = np.full(n, np.inf) if up is None else np.asarray(up, dtype=np.float64)
    return (lo if lo.ndim == 1 else lo[k]), (up if up.ndim == 1 else up[k])


def reference(fam, x, C, tq, lo=None, up=None, eps=None):
    """numpy float64 at the given (rounded) inputs: value, sigma and the uncancelled magnitude sqrt(sum g_j^2 C_jj), each count x q.
    A fixed parameter (l == u) is left out; one whose central difference is clipped to one side by the box (with eps, the
    step) takes the one-sided float64 difference as its derivative."""
    x = np.asarray(x, dtype=np.float64); C = np.asarray(C, dtype=np.float64); tq = np.asarray(tq, dtype=np.float64)
    count, n = x.shape
    q = tq.shape[-1]
    val = np.empty((count, q)); sig = np.empty((count, q)); mag = np.empty((count, q))
    for k in range(count):
        t = tq if tq.ndim == 1 else tq[k]
        l, u = box_of(lo, up, k, n)
        val[k] = fam.value(t, x[k])
        g = fam.jacobian(t, x[k])
        free = l != u
        if eps is not None:
            for j in np.flatnonzero(free):
                a = x[k].copy(); b = x[k].copy()
                a[j] = min(x[k, j] + eps, u[j]); b[j] = max(x[k, j] - eps, l[j])
                if a[j] == x[k, j] or b[j] == x[k, j]:
                    g[:, j] = (fam.value(t, a) - fam.value(t, b)) / (a[j] - b[j])
        g = g[:, free]
        Ck = C[k][np.ix_(free, free)]
        sig[k] = np.sqrt(np.maximum(0.0, np.einsum("ij,jk,ik->i", g, Ck, g)))
        mag[k] = np.sqrt(np.einsum("ij,j->i", g * g, np.diag(Ck)))
    return val, sig, mag


def value_gap(v, ref):
    v = np.asarray(v, dtype=np.float64)
    return float(np.max(np.abs(v - ref) / np.maximum(np.abs(ref), 1e-3 * np.abs(ref).max(axis=-1, keepdims=True))))


def sigma_gap(s, ref, mag):
    return float(np.max(np.abs(np.asarray(s, dtype=np.float64) - ref) / mag))


def emulate(fam, dtype, x, C, tq, eps, analytic=False):
    """the kernel's arithmetic restated in numpy in `dtype` (unbounded): (value, sigma), count x q"""
    T = np.dtype(dtype).type
    x = np.asarray(x, dtype=T); C = np.asarray(C, dtype=T); tq = np.asarray(tq, dtype=T); eps = T(eps)
    count, n = x.shape
    val = np.empty((count, tq.shape[-1]), dtype=T); sig = np.empty_like(val)
    for k in range(count):
        t = tq if tq.ndim == 1 else tq[k]
        val[k] = fam.value(t, x[k])
        if analytic:
            g = fam.jacobian(t.astype(np.float64), x[k].astype(np.float64)).astype(T)       # (the derivative's own rounding aside)
        else:
            g = np.empty((t.size, n), dtype=T)
            for j in range(n):
                a = x[k].copy(); b = x[k].copy()
                a[j] = x[k, j] + eps; b[j] = x[k, j] - eps
                g[:, j] = (fam.value(t, a) - fam.value(t, b)) * (T(1) / (a[j] - b[j]))
        inner = g @ C[k].T
        s = np.sum(g * inner, axis=1, dtype=T)
        sig[k] = np.sqrt(np.maximum(T(0), s))
    return val, sig


def cpu_figures(name, dtype, q=129):
    """{kind: worst gap} of emulate() against reference() for a family: 'value', 'fd', 'analytic'"""
    fam = family(name)
    x, C, tq = fam.x.astype(dtype), fam.C.astype(dtype), grid(q, dtype)
    vr, sr, mag = reference(fam, x, C, tq)
    out = {}
    for kind in ("fd", "analytic"):
        v, s = emulate(fam, dtype, x, C, tq, EPS[dtype], analytic=kind == "analytic")
        out["value"] = value_gap(v, vr)
        out[kind] = sigma_gap(s, sr, mag)
    return out


def round_up_one_digit(v):
    return WP16.round_up_one_digit(v)


def min_eig_ratio(name, dtype):
    """smallest over largest eigenvalue of the dtype cast of the family's covariances, the worst of the set (positive: definite)"""
    fam = family(name)
    ev = [np.linalg.eigvalsh(fam.C[k].astype(dtype).astype(np.float64)) for k in range(COUNT)]
    return min(float(e.min() / e.max()) for e in ev)


# What cpu_figures() gave (q = 129, numpy 1.x / 2.x on x86-64; rounded up to two digits; "below 1e-15" is entered as 1e-15).
# (family, dtype name): {kind: figure}
CPU_FIGURE = {
    ("exp_decay", "float32"): {"value": 1.8e-7, "fd": 3.3e-4, "analytic": 1.3e-7},
    ("exp_decay", "float64"): {"value": 1e-15, "fd": 2.0e-8, "analytic": 1e-15},
    ("exp3", "float32"): {"value": 2.7e-7, "fd": 1.4e-3, "analytic": 1.2e-5},
    ("exp3", "float64"): {"value": 1e-15, "fd": 7.6e-8, "analytic": 2.9e-14},
    ("pad8", "float32"): {"value": 1.1e-5, "fd": 4.6e-4, "analytic": 5.5e-6},
    ("pad8", "float64"): {"value": 1e-15, "fd": 2.7e-8, "analytic": 1.6e-14},
    ("peak", "float32"): {"value": 1.5e-7, "fd": 3.3e-4, "analytic": 1.1e-7},
    ("peak", "float64"): {"value": 1e-15, "fd": 2.1e-8, "analytic": 1e-15},
    ("harm9", "float64"): {"value": 1e-15, "fd": 7.2e-8, "analytic": 1.1e-15},
    ("harm13", "float64"): {"value": 1e-15, "fd": 8.6e-8, "analytic": 1.4e-15},
    ("harm16", "float64"): {"value": 1e-15, "fd": 1.2e-7, "analytic": 9.7e-15},
    ("gauss3", "float64"): {"value": 1e-15, "fd": 1.1e-8, "analytic": 1e-15},
}


def bar(fam_name, dtype, kind, device_gap):
    """10 x the larger of the device's measured worst gap and the CPU figure, rounded up to one digit"""
    return round_up_one_digit(10 * max(device_gap, CPU_FIGURE[(fam_name, np.dtype(dtype).name)][kind]))
