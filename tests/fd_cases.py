"""Cells and references for the finite-difference and bookkeeping kernels of csrc/misc_kernels.h, one launch at a time through
M.fdPoints, M.fdFill, M.entryState and M.unpackGrad (tests/test_gpu_fd_cells.py runs them on the device,
tests/test_decide_cell_coverage.py holds the references to slow per-element loops on the CPU).

Everything but the random sums of squares is compared BIT FOR BIT with numpy in the cell's type: the points are one addition and
one fmin / fmax (LS:1027-1031), a Jacobian entry is one subtraction and one multiplication by T(1) / twh (LS:1041-1047; contracting
a + (-1) b into an fma changes nothing, the product is exact), the unpacking copies, and sums of exact integers are exact in any order.

THE BOUND of a random sum of squares: all terms are positive, so a summation tree whose longest chain of roundings is d is within
gamma_d = d u / (1 - d u) of the exact sum, relatively (u the unit roundoff of the type). The chain, from the kernels:
  stage 1 (k_sumsq_partial, nb = ceil(m / 4096) workgroups, at most kPartials = 1024, of 256 threads over ceil(m / nb) rows):
      1 (the product; 0 when it is fused into the addition) + ceil(ceil(m / nb) / 256) additions of a thread's strided walk
      + 6 (the wave's butterfly) + 2 (the four waves: (r0 + r1) + (r2 + r3))
  stage 2 (k_sumsq_final, one workgroup of 256 threads over the nb partials): ceil(nb / 256) + 6 + 2.
`chain_length(m)` is that sum; the reference (math.fsum of the squares in double) adds one rounding of its own per square in
double, which `bound` adds as 2 u_64 (nothing beside u in single precision)."""
import math

import numpy as np

from mir_optim_amd import api

DTYPES = (np.float32, np.float64)
EPS = 2.0 ** -20
EPS_LARGE = 1000.0
POINT_NS = (1, 2, 63, 64, 65, 300)
FILL_MS = (1, 63, 64, 65, 200)
FILL_NS = (1, 31, 32, 33, 70)
FILL_SENTINEL = -654321.0
STATE_MS = (1, 255, 257, 4095, 4096, 4097, 131077)
UNPACK_NS = (1, 2, 127, 128, 129, 300)
KPARTIALS = 1024


# ---------------------------------------------------------------------------------------------------------------- fd_points
def points_inputs(n, dtype, bounds, shift=0):
    """x, lower, upper. bounds = "inf": no bound; "finite": coordinate j is, by (j + shift) % 6: interior / at the upper bound /
    at the lower bound / within EPS / 2 of the upper bound / lower == upper == x (a collapsed interval) / within EPS / 2 of the lower"""
    T = np.dtype(dtype).type
    j = np.arange(n)
    x = (((j - n // 2) * 0.37 + 0.1) / n).astype(dtype)          # |x| < 1: EPS is many units in the last place of x in both types
    lo, up = np.full(n, -np.inf, dtype=dtype), np.full(n, np.inf, dtype=dtype)
    if bounds == "finite":
        kind = (j + shift) % 6
        h = T(EPS / 2)
        lo = np.where(kind == 2, x, np.where(kind == 4, x, np.where(kind == 5, x - h, x - T(1)))).astype(dtype)
        up = np.where(kind == 1, x, np.where(kind == 4, x, np.where(kind == 3, x + h, x + T(1)))).astype(dtype)
    return x, lo, up


def points_reference(x, lo, up, eps, with_base):
    T = x.dtype.type
    n = x.size
    xmh, xph = np.fmax(x - T(eps), lo), np.fmin(x + T(eps), up)                       # LS:1028-1031
    X = np.tile(x, (2 * n + (1 if with_base else 0), 1))
    X[2 * np.arange(n), np.arange(n)] = xph
    X[2 * np.arange(n) + 1, np.arange(n)] = xmh
    return X, xph - xmh


def points_reference_slow(x, lo, up, eps, with_base):
    T = x.dtype.type
    n = x.size
    X, twh = np.zeros((2 * n + (1 if with_base else 0), n), dtype=x.dtype), np.zeros(n, dtype=x.dtype)
    for j in range(n):
        save = x[j]
        xmh, xph = save - T(eps), save + T(eps)
        xmh = lo[j] if lo[j] > xmh else xmh
        xph = up[j] if up[j] < xph else xph
        for k in range(n):
            X[2 * j, k] = xph if k == j else x[k]
            X[2 * j + 1, k] = xmh if k == j else x[k]
        twh[j] = xph - xmh
    if with_base:
        X[2 * n] = x
    return X, twh


# ---------------------------------------------------------------------------------------------------------------- fd_fill
def panels(n):
    """the whole panel and the sub-panels (j0, pc) that fit n columns"""
    out = [(0, n)]
    for j0, pc in ((0, 1), (5, 32), (33, 37), (n - 1, 1)):
        if j0 >= 0 and j0 + pc <= n and (j0, pc) not in out:
            out.append((j0, pc))
    return out


def collapsed_columns(m, j0, pc):
    """two collapsed columns in a panel of three or more, else the panel's first column for odd m + j0"""
    if pc >= 3:
        return {j0 + 1, j0 + pc - 1}
    return {j0} if (m + j0) % 2 else set()


def fill_inputs(m, n, j0, pc, ldy, dtype, special=False, seed=0):
    """Y (2 pc x ldy; the rows of collapsed columns and the padding behind m hold NaN: the host never evaluates them), twh (n; NaN
    outside the panel: not read), J (the sentinel everywhere)"""
    rng = np.random.default_rng(seed + 1000 * m + n)
    Y = rng.standard_normal((2 * pc, ldy)).astype(dtype)
    Y[:, m:] = np.nan
    twh = np.full(n, np.nan, dtype=dtype)
    twh[j0:j0 + pc] = (2.0 ** -19 * (1 + rng.integers(0, 8, pc) / 8.0) * np.where(rng.random(pc) < 0.3, 0.5, 1.0)).astype(dtype)
    for j in collapsed_columns(m, j0, pc):
        twh[j] = 0
        Y[2 * (j - j0):2 * (j - j0) + 2] = np.nan
    if special:                                                # +-inf and NaN in live rows propagate as numpy's do
        live = [c for c in range(pc) if twh[j0 + c] != 0]
        Y[2 * live[0], 0], Y[2 * live[0] + 1, m - 1], Y[2 * live[1], m // 2] = np.inf, -np.inf, np.nan
        Y[2 * live[2], 1], Y[2 * live[2] + 1, 1] = np.inf, np.inf
    return Y, twh, np.full((m, n), FILL_SENTINEL, dtype=dtype)


def fill_reference(Y, twh, J, j0, pc):
    T = J.dtype.type
    m = J.shape[0]
    out = J.copy()
    with np.errstate(all="ignore"):
        for c in range(pc):
            t = twh[j0 + c]
            out[:, j0 + c] = (Y[2 * c, :m] - Y[2 * c + 1, :m]) * (T(1) / t) if t != 0 else T(0)      # LS:1041-1047
    return out


def fill_reference_slow(Y, twh, J, j0, pc):
    T = J.dtype.type
    out = J.copy()
    with np.errstate(all="ignore"):
        for i in range(J.shape[0]):
            for c in range(pc):
                t = twh[j0 + c]
                if t != 0:
                    d = Y[2 * c, i]
                    d = d + T(-1) * Y[2 * c + 1, i]
                    out[i, j0 + c] = d * (T(1) / t)
                else:
                    out[i, j0 + c] = T(0)
    return out


# ---------------------------------------------------------------------------------------------------------------- entry state
def blocks_by_hand(m):
    return max(1, min(KPARTIALS, (m + 4095) // 4096))


def chain_length(m, fused=False):
    nb = blocks_by_hand(m)
    per = -(-m // nb)
    return (0 if fused else 1) + -(-per // 256) + 6 + 2 + -(-nb // 256) + 6 + 2


def bound(m, dtype):
    u = np.finfo(dtype).eps / 2
    d = chain_length(m)
    return d * u / (1 - d * u) + 2 * np.finfo(np.float64).eps / 2


def exact_vectors(m, dtype, seed=0):
    """2 x m integers in [-3, 3]: every square and every partial sum (at most 9 m < 2^24) is exact in both types"""
    return np.random.default_rng(seed + m).integers(-3, 4, (2, m)).astype(dtype)


def random_vectors(m, dtype, seed=0):
    return np.random.default_rng(seed + 7 * m).standard_normal((2, m)).astype(dtype)


def fsum_squares(v):
    v = v.astype(np.float64)
    return math.fsum((v * v).tolist())


def _butterfly(s):
    """a wave's sum: 64 lanes, partners at distance 8, 4, 2, 1, 16, 32 (every lane ends with the total)"""
    for d in (8, 4, 2, 1, 16, 32):
        s = s + s[np.arange(64) ^ d]
    return s[0]


def _block_sum(vals):
    """256 threads' values -> (w0 + w1) + (w2 + w3)"""
    w = [_butterfly(vals[64 * k:64 * k + 64]) for k in range(4)]
    return (w[0] + w[1]) + (w[2] + w[3])


def tree_sum_squares(v, order="kernel"):
    """the two-stage tree in numpy, in the type of v. "kernel": the kernels' order; "reversed": every thread walks its rows
    backwards and the partials come in reverse; "pairwise": numpy's own pairwise sum inside each workgroup's chunk and over the partials"""
    T = v.dtype.type
    m = v.size
    nb = blocks_by_hand(m)
    per = -(-m // nb)
    parts = []
    for b in range(nb):
        chunk = v[b * per:min(b * per + per, m)]
        sq = chunk * chunk
        if order == "pairwise":
            parts.append(sq.sum(dtype=v.dtype) if sq.size else T(0))
            continue
        rows = -(-max(sq.size, 1) // 256)
        pad = np.zeros(rows * 256, dtype=v.dtype)
        pad[:sq.size] = sq
        pad = pad.reshape(rows, 256)
        if order == "reversed":
            pad = pad[::-1]
        s = np.zeros(256, dtype=v.dtype)
        for r in range(rows):
            s = s + pad[r]
        parts.append(_block_sum(s))
    parts = np.array(parts[::-1] if order == "reversed" else parts, dtype=v.dtype)
    if order == "pairwise":
        return parts.sum(dtype=v.dtype)
    rows = -(-nb // 256)
    pad = np.zeros(rows * 256, dtype=v.dtype)
    pad[:nb] = parts
    s = np.zeros(256, dtype=v.dtype)
    for r in range(rows):
        s = s + pad.reshape(rows, 256)[r]
    return _block_sum(s)


def distinct_state(dtype):
    st = np.zeros(1, dtype=api.lm_state_dtype(dtype))
    for i, k in enumerate(st.dtype.names):
        st[k] = 3 + 2 * i
    return st


# ---------------------------------------------------------------------------------------------------------------- unpack_grad
UNPACK_MAX = ("first", "last", "negative", "zero")


def unpack_inputs(n, dtype, where):
    """the packed buffer [lower triangle of J^T J by rows | J^T y] with distinct values, the maximum of |J^T y| placed by `where`"""
    nt = n * (n + 1) // 2
    packed = (np.arange(nt + n) + 1.0).astype(dtype)                                  # < 2^24: exact in both types
    jy = -(np.arange(n) % 7 + 1.0) * np.where(np.arange(n) % 2, 1, -1)
    if where == "zero":
        jy[:] = 0
    else:
        jy[{"first": 0, "last": n - 1, "negative": n // 2}[where]] = -1e6 if where == "negative" else 1e6
    packed[nt:] = jy
    return packed


def unpack_reference(packed, n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    r, c = np.maximum(i, j), np.minimum(i, j)
    nt = n * (n + 1) // 2
    Jy = packed[nt:].copy()
    return packed[r * (r + 1) // 2 + c], Jy, np.abs(Jy).max()
