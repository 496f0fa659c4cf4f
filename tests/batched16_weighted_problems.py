"""Problem sets and the numpy reference of the weighted batched fits with 9 to 16 parameters (tests/test_batched16_weighted_host.py,
tests/test_gpu_batched16_weighted.py, scripts/batched16.py; not a test module). The families of tests/batched16_problems.py --
same seeds 700 + k, truths and starts -- made heteroscedastic by the recipe of tests/weighted_problems.py:
    sigma = 0.01 sqrt(|clean| / max |clean|) + 0.002,   w = 1 / sigma,   data = clean + 1.7 sigma (2 u[2 n:] - 1)
Every fourth problem has 37 weights set to 0: the harmonic family in rows m // 3 .. m // 3 + 36 (zero="tail": the last 37 rows,
for the comparison with truncated problems), the three-Gaussian family in rows 1, 4, .., 109 (a contiguous block there removes
a peak's support and makes J^T J singular). A set with m - 37 < 4 n (the small m of the GPU cases: m = 2 n + 1 and 67) has no zero
weights: 30 rows around a gap leave 13 harmonics a J^T J of condition 1e9, on which the oracle disagrees with itself.
Also the float64 model Jacobians, and what the reference side gives on its own for a set: the condition number of the
equilibrated J^T J and the covariance gap of central differences at h = 2^-26 against the analytic Jacobian (reference_figures);
the covariance bars of the GPU test are built from those (CPU_FD_GAP, which the host test holds to what it recomputes)."""
import functools

import numpy as np

import problems as P
from batched16_problems import COUNT, gauss3_value, harm_basis, harm_problems, harm_value
from weighted_problems import ZERO_TAIL, _sigma, reference_covariance, scaled_gap      # noqa: F401  (re-exported)

H = 2.0 ** -26                 # jacobianEpsilon of the default settings


def _zero_rows(n, m, zero):
    if m - ZERO_TAIL < 4 * n:
        return np.arange(0)
    return np.arange(m - ZERO_TAIL, m) if zero == "tail" else np.arange(m // 3, m // 3 + ZERO_TAIL)


@functools.lru_cache(maxsize=None)
def harm_weighted(n, m, count=COUNT, zero="middle"):
    """(t, B, data, x0, w) of the weighted harmonic set; t, B and x0 are those of harm_problems(n, m, count)"""
    t, B, _, truth, x0 = harm_problems(n, m, count)
    data = np.empty((count, m)); w = np.empty((count, m))
    rows = _zero_rows(n, m, zero)
    for k in range(count):
        u = P.splitmix64_uniform(700 + k, m + 2 * n)
        clean = harm_value(B, t, truth[k])
        sigma = _sigma(clean)
        w[k] = 1.0 / sigma
        data[k] = clean + 1.7 * sigma * (2 * u[2 * n:] - 1)
        if k % 4 == 0:
            w[k, rows] = 0.0
    for a in (data, w):
        a.setflags(write=False)
    return t, B, data, x0, w


GAUSS3_ZERO_ROWS = np.arange(1, 110, 3)          # 37 rows


@functools.lru_cache(maxsize=None)
def gauss3_weighted(m=130, count=COUNT):
    """(t, data, x0, w) of the weighted three-Gaussian set (n = 11); t and x0 are those of gauss3_problems(m, count)"""
    t = np.linspace(0.0, 4.0, m)
    n = 11
    data = np.empty((count, m)); x0 = np.empty((count, n)); w = np.empty((count, m))
    for k in range(count):
        u = P.splitmix64_uniform(700 + k, m + 2 * n)
        p = np.array([1 + u[0], 0.8 + 0.2 * u[1], 0.15 + 0.1 * u[2], 1 + u[3], 2.0 + 0.2 * u[4], 0.15 + 0.1 * u[5],
                      1 + u[6], 3.1 + 0.2 * u[7], 0.15 + 0.1 * u[8], 0.2 * u[9], 0.1 * u[10] - 0.05])
        x0[k] = p * (1 + 0.1 * (2 * u[n:2 * n] - 1))
        clean = gauss3_value(t, p)
        sigma = _sigma(clean)
        w[k] = 1.0 / sigma
        data[k] = clean + 1.7 * sigma * (2 * u[2 * n:] - 1)
        if k % 4 == 0:
            w[k, GAUSS3_ZERO_ROWS] = 0.0
    for a in (t, data, x0, w):
        a.setflags(write=False)
    return t, data, x0, w


def harm_jacobian(B, t, p):
    """d harm_value / d p, m x n, float64"""
    e = np.exp(-t * p[1])
    return np.concatenate([np.stack([e, -t * p[0] * e, np.ones_like(t)], axis=1), B.T], axis=1)


def gauss3_jacobian(t, p):
    """d gauss3_value / d p, m x 11, float64"""
    cols = []
    for k in range(3):
        a, c, s = p[3 * k:3 * k + 3]
        z = (t - c) / s
        e = np.exp(-0.5 * z * z)
        cols += [e, a * e * z / s, a * e * z * z / s]
    return np.stack(cols + [np.ones_like(t), t], axis=1)


def model_of(key):
    """key: ("harm", n, m) or ("gauss3", 11, m) -> (t, data, x0, w, value(p), jacobian(p)), value and jacobian on the set's t"""
    family, n, m = key
    if family == "harm":
        t, B, data, x0, w = harm_weighted(n, m)
        return t, data, x0, w, (lambda p: harm_value(B, t, p)), (lambda p: harm_jacobian(B, t, p))
    t, data, x0, w = gauss3_weighted(m)
    return t, data, x0, w, (lambda p: gauss3_value(t, p)), (lambda p: gauss3_jacobian(t, p))


def equilibrated_cond(J):
    """condition number of D J^T J D, D = diag(J^T J)^-1/2"""
    A = J.T @ J
    d = 1.0 / np.sqrt(np.diag(A))
    return float(np.linalg.cond(A * np.outer(d, d)))


def fd_jacobian(value, p, h=H):
    """central differences of the model at step h, float64"""
    J = np.empty((value(p).size, p.size))
    for j in range(p.size):
        a = p.copy(); b = p.copy()
        a[j] += h; b[j] -= h
        J[:, j] = (value(a) - value(b)) / (a[j] - b[j])
    return J


def reference_figures(key, xs):
    """(largest equilibrated condition number, worst covariance gap of central differences at H against the analytic Jacobian)
    of a set at the points xs (count x n), all in numpy float64"""
    t, data, x0, w, value, jac = model_of(key)
    cond = gap = 0.0
    for k, p in enumerate(np.asarray(xs, dtype=np.float64)):
        J = jac(p)
        r = w[k] * (value(p) - data[k])
        ref = reference_covariance(J, w[k], r @ r)
        cond = max(cond, equilibrated_cond(J * w[k][:, None]))
        gap = max(gap, scaled_gap(reference_covariance(fd_jacobian(value, p), w[k], r @ r), ref))
    return cond, gap


# The sets of the two test files, and the covariance gap of float64 central differences against the analytic Jacobian at the
# oracle's minimisers of each, as tests/test_batched16_weighted_host.py measures it (rounded up to two digits). The figure is
# the rounding noise of differences at h = 2^-26, which moves with the exp / sin / cos of the host's numpy: that test fails when
# what it recomputes is more than twice a figure here or less than half of it. The finite-difference covariance bars of the GPU test
# are 10 x these, rounded up to one digit.
SETS = [("harm", 16, 512), ("harm", 16, 131), ("harm", 13, 131), ("harm", 9, 131), ("gauss3", 11, 130),
        ("harm", 16, 67), ("harm", 16, 33), ("harm", 13, 67), ("harm", 9, 67)]
CPU_FD_GAP = {("harm", 16, 512): 8.3e-8, ("harm", 16, 131): 1.5e-7, ("harm", 13, 131): 1.5e-7, ("harm", 9, 131): 7.5e-8,
              ("gauss3", 11, 130): 1.1e-8, ("harm", 16, 67): 1.7e-7, ("harm", 16, 33): 1.8e-7, ("harm", 13, 67): 1.1e-7,
              ("harm", 9, 67): 6.0e-8}


def round_up_one_digit(v):
    e = np.floor(np.log10(v))
    return float(np.ceil(v / 10 ** e - 1e-12) * 10 ** e)


def fd_bar(key):
    return round_up_one_digit(10 * CPU_FD_GAP[key])


_ORACLE = {}


def oracle_fits(oracle, key, weighted=True, reverse=False, analytic=False, box=None, zero="middle", count=COUNT):
    """the oracle's float64 fits of a set on the WEIGHTED objective (weighted=False: the same data with weights of one),
    computed once and shared: [(result, x)]. reverse: the rows in the opposite order (another summation order). analytic: the
    oracle is given g = w J. box: (lower, upper, starts). Harmonic sets take zero= and count= as harm_weighted does."""
    ck = (key, weighted, reverse, analytic, box is not None, zero, count)
    if ck not in _ORACLE:
        family, n, m = key
        if family == "harm":
            t, B, data, x0, w = harm_weighted(n, m, count, zero)
            value, jac = (lambda tt, BB, p: harm_value(BB, tt, p)), (lambda tt, BB, p: harm_jacobian(BB, tt, p))
        else:
            t, data, x0, w = gauss3_weighted(m, count)
            B = np.zeros((0, m))
            value, jac = (lambda tt, BB, p: gauss3_value(tt, p)), (lambda tt, BB, p: gauss3_jacobian(tt, p))
        lo, up, starts = box if box is not None else (None, None, x0)
        if not weighted:
            w = np.ones_like(w)
        if reverse:
            t, B, data, w = t[::-1].copy(), B[:, ::-1].copy(), data[:, ::-1].copy(), w[:, ::-1].copy()
        out = []
        for k in range(count):
            def f(p, y, k=k):
                y[:] = w[k] * (value(t, B, p) - data[k])

            def g(p, J, k=k):
                J[:, :] = w[k][:, None] * jac(t, B, p)
            out.append(oracle.optimize(f, m, starts[k], lower=lo, upper=up, g=g if analytic else None, dtype=np.float64))
        _ORACLE[ck] = out
    return _ORACLE[ck]
