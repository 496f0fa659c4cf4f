"""Cells, data, references and named assertions for the model-residual kernels of csrc/workloads.hip and csrc/workloads_gemm.hip,
run ONE call of a C entry at a time between guard bands (tests/test_gpu_model_cells.py), and the inputs of the tanh test
(tests/test_gpu_tanh_cells.py). tests/test_model_cell_coverage.py keeps on the CPU that the cells reach every instantiated kernel,
that the data is what this text says, and that the assertions catch planted mistakes.

THE METHOD. The kernels sum a . x in orders this file does not want to know (16-lane DPP trees, MFMA chains with a permuted K
index, forked chains). So the EXACT tier makes the order irrelevant: A = Ai 2^-ea and X = Xi 2^-ex with integers Ai, Xi in -8..8
and ea + ex = e = round(log2(24 sqrt(n))), so that every product and every partial sum is an integer multiple of 2^-e below 2^53
(2^24 in float: |sum| <= 128 * 8 * 512 = 2^19 units) -- exact in any order, any fragment permutation, fused or not. s = a . x is
then known exactly on the host from the integer product, and the expected output is fl(T(s) - b) BIT FOR BIT, where T is the
device's own dtanh taken from the unary entry (W.unary) on the distinct values of s: the GEMM, its indexing and its edges are held
to the bit, and T itself is held to tanh by tests/test_gpu_tanh_cells.py. One row of Ai is multiplied by 16 (m >= 64: at most 1/64
of the outputs, so the share of saturated ones stays below 2 %), which reaches saturation and the clamp; one row is zero (m >= 3).

THE REAL-VALUED tier runs the same entries on data like tests/problems.py's (uniform rows scaled by sqrt(3 / n), points near x*)
and on that data times 8, against a long-double reference. First-order bound of one output y = fl(T(fl_sum(a . x)) - b):
  * the sum: any order of n products, fused or not, errs by at most (n - 1 + 1) u S with S = sum |a_j x_j|, u = 2^-53 (each of the
    at most n roundings -- n - 1 additions and, unfused, the product, which a fused step merges -- is relative u of a partial
    result bounded by S); |tanh'| <= 1 carries it to the output unamplified: n u S;
  * T: E_T (test_gpu_tanh_cells.py);
  * the subtraction: u |t - b| <= u (|t| + |b|).
  real_bound = n u S + E_T + u (|t| + |b|). A difference-panel entry is the rounded difference of two such outputs: the sum of
  their two bounds plus u |d|.
"""
import collections
import fractions
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
# E_T: the bound of |dtanh(x) - tanh(x)| derived in tests/test_gpu_tanh_cells.py (27 * 2^-56 = 3.375 u, and the reference's own 2^-62)
E_T = 27 * 2.0 ** -56 + 2.0 ** -62
LOG2E = 1.4426950408889634            # the constant of dtanh
GUARD = 16                            # canary elements in front of and behind every output (128 bytes: keeps 16-byte alignment)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def canary(count, dtype, salt=0):
    """a NaN-free pattern no kernel writes: distinct values around -3e5"""
    return (-(2.0 ** 18) - 0.25 - np.arange(count) - 1000.0 * salt).astype(dtype)


# ------------------------------------------------------------------------------------------------------------ tanh inputs
def neighbours(c, k=8):
    out = [np.float64(c)]
    lo = hi = np.float64(c)
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.array(sorted(out))


def rint_boundary(k):
    """|x| at which dtanh's exponent index rint(2 |x| log2 e) goes from k to k + 1"""
    return (k + 0.5) / LOG2E / 2


def tanh_magnitudes():
    """the |x| of test_gpu_tanh_cells.py (every one goes in with both signs): +0, the smallest and the largest denormal, 2^-k for
    k = 1..1074, 200 000 log-uniform values in 1e-30..40, the neighbourhoods (8 values on either side) of the 59 rounding
    boundaries of the exponent index, of the clamp |x| = 20 and of |x| = 19.06 (where tanh rounds to 1), 1e300 and infinity"""
    rng = np.random.default_rng(23)
    parts = [np.array([0.0, 5e-324, np.nextafter(np.finfo(np.float64).tiny, 0.0), 1e300, np.inf]),
             np.ldexp(1.0, -np.arange(1, 1075)),
             np.exp(rng.uniform(np.log(1e-30), np.log(40.0), 200000))]
    parts += [neighbours(rint_boundary(k)) for k in range(59)] + [neighbours(20.0), neighbours(19.06)]
    return np.unique(np.concatenate(parts))


# ------------------------------------------------------------------------------------------------------------ rounding helpers
def round_fraction(fr, dtype):
    """the Fraction fr rounded to nearest-even in dtype (normal range)"""
    if dtype == np.float64:
        return np.float64(float(fr))             # int / int true division is correctly rounded
    if fr == 0:
        return np.float32(0)
    sign, fr = (-1 if fr < 0 else 1), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length() - 24
    while fr >= fractions.Fraction(2) ** (e + 24):
        e += 1
    while fr < fractions.Fraction(2) ** (e + 23):
        e -= 1
    q = fr / fractions.Fraction(2) ** e            # in [2^23, 2^24)
    k = q.numerator // q.denominator
    rem = q - k
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and k % 2):
        k += 1
    return np.float32(sign * math.ldexp(k, e))


def one_minus_square(t):
    """(separate, fused): fl(1 - fl(t t)) and fl(1 - t t) for every element of t, in t's type"""
    sep = (t.dtype.type(1) - t * t).astype(t.dtype)
    fused = np.array([round_fraction(1 - fractions.Fraction(float(v)) ** 2, t.dtype.type) for v in t.ravel()], dtype=t.dtype).reshape(t.shape)
    return sep, fused


def fma_exact(a, b, c, dtype):
    """fl(a b + c), one rounding"""
    return round_fraction(fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c)), dtype)


# ------------------------------------------------------------------------------------------------------------ tanh-linear data
def scale_exponents(n):
    e = int(round(math.log2(24 * math.sqrt(n))))
    return e // 2, e - e // 2


Data = collections.namedtuple("Data", "A X b S e")        # S: the integer sums (m x p), s = S 2^-e; None for real-valued data


def exact_data(m, n, p, dtype=np.float64, seed=0, fd=None, base=False):
    """fd: None -- p random points; else the finite-difference structure on an integer base point: points 2 j and 2 j + 1 are
    x +- one unit at coordinate j, with the minus point clamped onto x where j % 7 == 1, the plus point where j % 7 == 2 and both
    where j == 5 (a collapsed interval); p = 2 n. base: one more point behind them, x itself."""
    rng = np.random.default_rng([seed, m, n, p])
    ea, ex = scale_exponents(n)
    Ai = rng.integers(-8, 9, (m, n))
    if m >= 64:
        Ai[m // 2] *= 16
    if m >= 3:
        Ai[m // 3] = 0
    if fd is None:
        Xi = rng.integers(-8, 9, (p + (1 if base else 0), n))
    else:
        assert p == 2 * n
        x = rng.integers(-8, 9, n)
        Xi = np.repeat(x[None, :], 2 * n + (1 if base else 0), axis=0)
        j = np.arange(n)
        plus = np.where((j % 7 == 2) | (j == 5), 0, 1)
        minus = np.where((j % 7 == 1) | (j == 5), 0, 1)
        Xi[2 * j, j] += plus
        Xi[2 * j + 1, j] -= minus
    S = Ai @ Xi.T
    A = np.ldexp(Ai.astype(np.float64), -ea).astype(dtype)
    X = np.ldexp(Xi.astype(np.float64), -ex).astype(dtype)
    b = rng.standard_normal(m).astype(dtype)
    return Data(A, X, b, S, ea + ex)


def real_data(m, n, p, scale=1.0, seed=0, base=False):
    rng = np.random.default_rng([seed, m, n, p, 77])
    A = rng.uniform(-1, 1, (m, n)) * math.sqrt(3.0 / n) * scale
    xs = rng.uniform(-1, 1, n)
    X = xs[None, :] + 0.1 * rng.uniform(-1, 1, (p + (1 if base else 0), n))
    b = np.tanh(A @ xs / scale) + 1e-3 * rng.uniform(-1, 1, m)
    return Data(A, X, b, None, None)


def sums(d, dtype=np.float64):
    """s = a . x of exact data, m x points, exact in dtype"""
    return np.ldexp(d.S.astype(np.float64), -d.e).astype(dtype)


def exact_conditions(d):
    """what the coverage test asserts of every exact cell: the sums are exact (two summation orders in the cell's type and the
    integer product agree), at most 2 % of them saturated (|s| >= 19.06), at least 25 % with |s| < 2"""
    dt = d.A.dtype.type
    s = sums(d, dt)
    fwd = np.zeros(s.shape, dtype=dt)
    bwd = np.zeros(s.shape, dtype=dt)
    n = d.A.shape[1]
    for j in range(n):
        fwd = (fwd + d.A[:, j, None] * d.X[None, :, j]).astype(dt)
        k = n - 1 - j
        bwd = (bwd + d.A[:, k, None] * d.X[None, :, k]).astype(dt)
    exact = same_bits(fwd, s) and same_bits(bwd, s) and np.array_equal(s.astype(np.float64) * 2.0 ** d.e, d.S)
    return exact, float(np.mean(np.abs(s) >= 19.06)), float(np.mean(np.abs(s) < 2))


# ------------------------------------------------------------------------------------------------------------ references
def residuals(t, b):
    """y[i, k] = fl(t[i, k] - b[i])"""
    return (t - b[:, None]).astype(t.dtype)


def layout(y, op, base=False):
    """the m x points residuals y as the entry `op` stores them (flat): f: the one column; fb: point-major; fbr: row-major;
    fbd: the row-major difference panel of the point pairs, then (base) the last point's residual vector"""
    if op == "f":
        return y[:, 0].copy()
    if op == "fb":
        return np.ascontiguousarray(y.T).ravel()
    if op == "fbr":
        return np.ascontiguousarray(y).ravel()
    pairs = y[:, :-1] if base else y
    d = (pairs[:, 0::2] - pairs[:, 1::2]).astype(y.dtype)
    return np.concatenate([d.ravel(), y[:, -1]]) if base else d.ravel()


def jacobian_candidates(t, A):
    """MODE 1: d a with d = 1 - t t in either rounding, (separate, fused), flat row-major"""
    sep, fused = one_minus_square(t)
    return [(d[:, None] * A).astype(A.dtype).ravel() for d in (sep, fused)]


def real_reference(d, op, base=False):
    """(reference, bound) of the real-valued tier in long double, laid out like layout()"""
    A, X, b = d.A.astype(LD), d.X.astype(LD), d.b.astype(LD)
    n = d.A.shape[1]
    s = A @ X.T
    S = np.abs(A) @ np.abs(X).T
    t = np.tanh(s)
    y = t - b[:, None]
    bound = n * U * S + E_T + U * (np.abs(t) + np.abs(b)[:, None])
    if op != "fbd":
        return layout(y, op), layout(bound, op)
    pairs_y, pairs_b = (y[:, :-1], bound[:, :-1]) if base else (y, bound)
    dref = pairs_y[:, 0::2] - pairs_y[:, 1::2]
    dbound = pairs_b[:, 0::2] + pairs_b[:, 1::2] + U * np.abs(dref)
    if base:
        return np.concatenate([dref.ravel(), y[:, -1]]), np.concatenate([dbound.ravel(), bound[:, -1]])
    return dref.ravel(), dbound.ravel()


# ------------------------------------------------------------------------------------------------------------ named assertions
def guarded(body, extra=0):
    """body between its guard bands as the device test lays an output out (extra: elements of back guard beyond GUARD)"""
    return np.concatenate([canary(GUARD, body.dtype, 1), body, canary(GUARD + extra, body.dtype, 2)])


def check_band(got_with_guards, want, count):
    """got_with_guards: GUARD canary elements, `count` outputs, GUARD canary elements (salts 1, 2). Raises AssertionError whose
    text begins with the name of what is wrong: front-guard, back-guard, or values."""
    dt = got_with_guards.dtype
    front, body, back = got_with_guards[:GUARD], got_with_guards[GUARD:GUARD + count], got_with_guards[GUARD + count:]
    assert same_bits(front, canary(GUARD, dt, 1)), "front-guard: written in front of the output"
    assert same_bits(back, canary(back.size, dt, 2)), "back-guard: written behind the output"
    if isinstance(want, list):                                  # any ONE candidate, whole
        ok = any(same_bits(body, w) for w in want)
        assert ok, "values: the output equals none of the %d admissible roundings as a whole (first differences %s)" % (
            len(want), [np.flatnonzero(bits(body) != bits(w))[:4].tolist() for w in want])
    else:
        bad = np.flatnonzero(bits(body) != bits(want))
        assert bad.size == 0, "values: %d of %d outputs differ, first at %s: got %s, want %s" % (
            bad.size, count, bad[:6].tolist(), body[bad[:3]].tolist(), want[bad[:3]].tolist())


def check_real(got, ref, bound):
    """Returns the largest error / bound; raises 'real-bound' if above 1."""
    err = np.abs(got.astype(LD) - ref)
    ratio = float(np.max(err / bound)) if got.size else 0.0
    assert ratio <= 1.0, "real-bound: error / bound = %.3f at output %d" % (ratio, int(np.argmax(err / bound)))
    return ratio


# ------------------------------------------------------------------------------------------------------------ the class by hand
def hand_class(op, m, n, p=1, a_A=0, a_x=0, a_y=0, elem=8, read_a_once=False, dense=False):
    """(family, width, flags, mode, launches) restated from the kernels' own conditions (the comments at each kernel and entry of
    workloads.hip / workloads_gemm.hip), not from tl_class"""
    def point(mode):
        if n > 256:
            return ("ROWS", 0, frozenset(), mode, 1)
        ncp = 1 if n <= 32 else 2 if n <= 64 else 4 if n <= 128 else 8
        vec = n % 2 == 0 and a_A % (2 * elem) == 0
        return ("SWEEP", ncp, frozenset(["VEC"] if vec else []), mode, 1)

    if op in ("f", "g"):
        return point(1 if op == "g" else 0)
    dma_n = {32: 8, 64: 16, 128: 32, 256: 64}
    wide = n > 256 and n % 8 == 0 and m > 0
    if op == "fb":
        if p <= 8 and n <= 128 and n % 2 == 0 and a_A == 0 and a_x == 0:
            return ("MULTI", 1 if n <= 32 else 2 if n <= 64 else 4, frozenset(), 0, 1)
        if n in dma_n and m >= 32:
            return ("DMA", dma_n[n], frozenset(["VEC"] if (m % 2 == 0 and a_y == 0) else []), 0, 1)
        if wide:
            return ("WIDE", 2, frozenset(), 0, 1)
        if n % 2 or n > 128 or n < 4:
            f = point(0)
            return ("LOOP", f[1], f[2], 0, p)
        return ("MFMA", 4 if n <= 16 else 8 if n <= 32 else 16 if n <= 64 else 32, frozenset(), 0, 1)
    if op == "fbr":
        if n in dma_n and m >= 32:
            return ("DMA", dma_n[n], frozenset(["RM"]), 0, 1)
        return ("WIDE", 0, frozenset(), 0, 1) if wide else ("GENERIC_RM", 0, frozenset(), 0, 1)
    base = p == 2 * n + 1
    P = 2 * n if base else p
    if n in dma_n and m >= 32 and P % 16 == 0:
        once = read_a_once and n <= 128 and P == 2 * n
        fork = (not read_a_once) and (not dense) and n == 128 and P == 2 * n
        mode = 1 if once else 2 if fork else 0
        if base and n == 128 and not read_a_once:
            return ("DMA", 32, frozenset(["RM", "DIFF", "BASE"]), mode, 1)
        return ("DMA", dma_n[n], frozenset(["RM", "DIFF"]), mode, 1 + base)
    if wide and P % 2 == 0:
        return ("WIDE", 1, frozenset(), 0, 1 + base)
    return ("GENERIC_DIFF", 0, frozenset(), 0, 1 + base)


# every instantiated tanh-linear kernel, written by hand from the launchers' template arguments: (kernel, type, arguments)
INSTANCES = set()
for _t in ("f64", "f32"):
    for _mode in (0, 1):
        INSTANCES.add(("k_tanh_linear_rows", _t, (_mode,)))
        for _ncp in (1, 2, 4, 8):
            for _vec in (True, False):
                INSTANCES.add(("k_tanh_linear", _t, (_ncp, _mode, _vec)))
for _w in (1, 2, 4):
    INSTANCES.add(("k_tanh_linear_multi", "f64", (_w, 8)))
for _w in (4, 8, 16, 32):
    INSTANCES.add(("k_tanh_linear_batched", "f64", (_w,)))
for _w in (8, 16, 32, 64):
    for _rm, _diff in ((False, False), (True, False), (True, True)):
        INSTANCES.add(("k_tanh_linear_batched_dma", "f64", (_w, _rm, _diff, False)))
INSTANCES.add(("k_tanh_linear_batched_dma", "f64", (32, True, True, True)))
for _o in (0, 1, 2):
    INSTANCES.add(("k_tanh_linear_batched_wide", "f64", (_o,)))
INSTANCES.add(("k_tanh_linear_batched_rm_generic", "f64", ()))
INSTANCES.add(("k_tanh_linear_batched_diff_generic", "f64", ()))
# paths inside the DMA kernel that are not template arguments: (NK, what)
DMA_PATHS = {(nk, w) for nk in (8, 16, 32, 64) for w in ("pm-aligned", "pm-unaligned", "rm", "diff-chunked")} \
    | {(nk, "diff-once") for nk in (8, 16, 32)} | {(32, "diff-fork"), (32, "base-fork"), (32, "base-dense")}


def instances_of(cls, dtype=np.float64):
    """the kernel instances a call of class cls (W.TlClass or hand_class's tuple) launches"""
    family, width, flags, mode, launches = cls
    t = "f64" if dtype == np.float64 else "f32"
    if family in ("SWEEP", "LOOP") and width:
        return {("k_tanh_linear", t, (width, mode, "VEC" in flags))}
    if family in ("ROWS", "LOOP"):
        return {("k_tanh_linear_rows", t, (mode,))}
    if family == "MULTI":
        return {("k_tanh_linear_multi", t, (width, 8))}
    if family == "MFMA":
        return {("k_tanh_linear_batched", t, (width,))}
    if family == "WIDE":
        return {("k_tanh_linear_batched_wide", t, (width,))}
    if family == "GENERIC_RM":
        return {("k_tanh_linear_batched_rm_generic", t, ())}
    if family == "GENERIC_DIFF":
        return {("k_tanh_linear_batched_diff_generic", t, ())}
    return {("k_tanh_linear_batched_dma", t, (width, "RM" in flags, "DIFF" in flags, "BASE" in flags))}


def dma_path(cls, dense=False):
    family, width, flags, mode, launches = cls
    if family != "DMA":
        return None
    if "BASE" in flags:
        return (width, "base-dense" if dense else "base-fork")
    if "DIFF" in flags:
        return (width, {0: "diff-chunked", 1: "diff-once", 2: "diff-fork"}[mode])
    if "RM" in flags:
        return (width, "rm")
    return (width, "pm-aligned" if "VEC" in flags else "pm-unaligned")


# ------------------------------------------------------------------------------------------------------------ the cells
# op, type, shape, element shifts of A / X / Y, the points ("random", "fd", "fd-broken": one coordinate of one point changed),
# read_a_once, dense
Cell = collections.namedtuple("Cell", "op dtype m n p sA sX sY points once dense")
SMALL_M = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65)
M_DMA2 = 32 * 256 + 33         # some DMA workgroups run a second stage, and the last stage is partial
M_MFMA3 = 8197                 # the point-major MFMA kernel's third pipeline round (256 workgroups x 16 rows x 2, and 5 rows)
M_RING = 81949                 # one-point sweep: 20488 row groups over 4096 waves, 6 a wave (no multiple of the ring of 4), the last waves short
SWEEP_N = (1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256)
ROWS_N = (257, 264, 512)


def cell(op, m, n, p=1, dtype=np.float64, sA=0, sX=0, sY=0, points="random", once=False, dense=False):
    return Cell(op, dtype, m, n, p, sA, sX, sY, points, once, dense)


def point_cells(op, dtype):
    """the one-point entries f and g: {n: [cells]}"""
    out = collections.OrderedDict()
    for n in SWEEP_N + ROWS_N:
        ms = SMALL_M if n <= 256 else (1, 5, 63, 64, 65, 200)
        out[n] = [cell(op, m, n, dtype=dtype) for m in ms]
        if n % 2 == 0 and n <= 256:
            out[n] += [cell(op, m, n, dtype=dtype, sA=1) for m in (5, 33)]       # A shifted by one element: not VEC
        if n in (32, 128):
            out[n] += [cell(op, M_DMA2, n, dtype=dtype), cell(op, M_MFMA3, n, dtype=dtype, sY=1)]
    if op == "f" and dtype == np.float64:
        out[30] = [cell("f", M_RING, 30)]
    return out


def fb_cells():
    out = collections.OrderedDict()
    multi = []
    for n in (2, 32, 34, 64, 66, 128):
        for p in (1, 2, 7, 8):
            multi += [cell("fb", m, n, p) for m in (1, 5, 33, 65)]
        multi += [cell("fb", 65, n, 9), cell("fb", 33, n, 2, sA=1), cell("fb", 33, n, 2, sX=1)]   # fall through: MFMA, DMA, LOOP
    multi += [cell("fb", 33, 33, 2), cell("fb", M_DMA2, 128, 8), cell("fb", M_DMA2, 32, 3)]
    out["multi"] = multi
    mfma = []
    for n in (4, 6, 16, 18, 30, 34, 62, 66, 126):
        mfma += [cell("fb", m, n, p) for m in (17, 65) for p in (9, 15, 16, 17, 255, 256, 257)]
        mfma += [cell("fb", m, n, p) for m in (1, 15, 16, 33) for p in (9, 17)]
    for n in (32, 64, 128):
        mfma += [cell("fb", m, n, p) for m in (5, 31) for p in (9, 16, 257)]
    mfma += [cell("fb", M_MFMA3, 16, 17), cell("fb", M_MFMA3, 126, 9, sY=1)]
    out["mfma"] = mfma
    dma = []
    for n in (32, 64, 128, 256):
        ps = (15, 16, 17, 127, 128, 129, 2 * n, 2 * n + 3)
        dma += [cell("fb", 64, n, p) for p in ps] + [cell("fb", 33, n, p) for p in ps]
        dma += [cell("fb", m, n, 17) for m in (32, 63, 65)] + [cell("fb", 64, n, 16, sY=1), cell("fb", 64, n, 9, sA=1), cell("fb", 64, n, 9, sX=1)]
        dma += [cell("fb", 64, n, 1, sA=1)]                    # p = 1 reaches the GEMM only when the sweep over a handful refuses
        if n <= 128:
            dma += [cell("fb", M_DMA2, n, 17), cell("fb", M_DMA2 + 1, n, 2 * n)]
    dma += [cell("fb", 64, 256, 1)]
    out["dma"] = dma
    wide = []
    for n in (264, 512):
        wide += [cell("fb", m, n, p) for m in (63, 64, 65) for p in (1, 2, 62, 64, 66, 130)] + [cell("fb", 1, n, 2), cell("fb", 200, n, 66, sY=1)]
    out["wide"] = wide
    out["loop"] = [cell("fb", 65, 33, 9), cell("fb", 33, 2, 9), cell("fb", 17, 130, 3), cell("fb", 31, 256, 2), cell("fb", 5, 257, 2),
                   cell("fb", 33, 127, 3, sA=1)]
    return out


def fbr_cells():
    out = collections.OrderedDict()
    dma = []
    for n in (32, 64, 128, 256):
        ps = (1, 15, 16, 17, 127, 128, 129, 2 * n, 2 * n + 3)
        dma += [cell("fbr", 64, n, p) for p in ps] + [cell("fbr", 33, n, p) for p in ps]
        dma += [cell("fbr", m, n, 17) for m in (32, 63, 65)] + [cell("fbr", 64, n, 16, sY=1), cell("fbr", 64, n, 9, sA=1), cell("fbr", 64, n, 9, sX=1)]
        if n <= 128:
            dma += [cell("fbr", M_DMA2, n, 17)]
    out["dma"] = dma
    wide = []
    for n in (264, 512):
        wide += [cell("fbr", m, n, p) for m in (63, 64, 65) for p in (1, 2, 62, 64, 66, 130)] + [cell("fbr", 1, n, 2), cell("fbr", 200, n, 66, sY=1)]
    out["wide"] = wide
    gen = []
    for n in (7, 33, 48):
        gen += [cell("fbr", m, n, p) for m in (1, 33, 65) for p in (1, 9, 17)]
    gen += [cell("fbr", 33, 257, 3), cell("fbr", 31, 32, 17), cell("fbr", 31, 128, 256)]
    out["generic"] = gen
    return out


def fbd_cells():
    out = collections.OrderedDict()
    dma = []
    for n in (32, 64, 128, 256):
        for m in (32, 33, 63, 64, 65):
            dma += [cell("fbd", m, n, 2 * n, dense=True), cell("fbd", m, n, 2 * n, points="fd"), cell("fbd", m, n, 2 * n, points="fd", dense=True)]
            dma += [cell("fbd", m, n, 2 * n, points="fd", once=True)]      # n = 256: not offered, the chunked sweep
        dma += [cell("fbd", 64, n, 16), cell("fbd", 33, n, 16, dense=True), cell("fbd", 65, n, 2 * n + 16), cell("fbd", 65, n, 2 * n + 16, once=True),
                cell("fbd", 64, n, 2 * n, sY=1), cell("fbd", 64, n, 2 * n, sA=1, points="fd"), cell("fbd", 64, n, 2 * n, sX=1, points="fd")]
        dma += [cell("fbd", 65, n, 2 * n + 1, points="fd"), cell("fbd", 65, n, 2 * n + 1, points="fd", dense=True),
                cell("fbd", 64, n, 2 * n + 1, points="fd", once=True), cell("fbd", 33, n, 2 * n + 1)]
        if n <= 128:
            dma += [cell("fbd", M_DMA2, n, 2 * n, points="fd"), cell("fbd", M_DMA2, n, 2 * n, points="fd", once=True),
                    cell("fbd", M_DMA2, n, 2 * n + 1, points="fd"), cell("fbd", M_DMA2, n, 2 * n + 1, points="fd", dense=True)]
    dma += [cell("fbd", m, 128, 256, points="fd-broken") for m in (33, 64, M_DMA2)] + [cell("fbd", 65, 128, 257, points="fd-broken")]
    out["dma"] = dma
    wide = []
    for n in (264, 512):
        wide += [cell("fbd", m, n, p) for m in (63, 64, 65) for p in (2, 62, 64, 66, 130)] + [cell("fbd", 1, n, 2), cell("fbd", 200, n, 66, sY=1)]
        wide += [cell("fbd", 65, n, 2 * n + 1, points="fd")]
    out["wide"] = wide
    gen = []
    for n in (7, 33, 48):
        gen += [cell("fbd", m, n, p) for m in (1, 33, 65) for p in (2, 2 * n, 2 * n + 1)]
    gen += [cell("fbd", 33, 257, 4), cell("fbd", 31, 32, 64, points="fd"), cell("fbd", 31, 128, 257, points="fd"), cell("fbd", 64, 32, 18)]
    out["generic"] = gen
    return out


def all_tanh_cells():
    out = []
    for op in ("f", "g"):
        for dt in (np.float64, np.float32):
            for cs in point_cells(op, dt).values():
                out += cs
    for group in (fb_cells(), fbr_cells(), fbd_cells()):
        for cs in group.values():
            out += cs
    return out


def cell_class_args(c):
    it = np.dtype(c.dtype).itemsize
    return dict(op=c.op, m=c.m, n=c.n, p=c.p, a_A=(c.sA * it) % 16, a_x=(c.sX * it) % 16, a_y=(c.sY * it) % 16, elem=it,
                read_a_once=c.once, dense=c.dense)


def cell_data(c, kind="exact"):
    base = c.op == "fbd" and c.p == 2 * c.n + 1
    p = c.p - 1 if base else c.p
    if kind != "exact":
        return real_data(c.m, c.n, p, scale=8.0 if kind == "real8" else 1.0, base=base)
    d = exact_data(c.m, c.n, p, c.dtype, fd=None if c.points == "random" else True, base=base)
    if c.points == "fd-broken":                                # point 255's chain takes coordinate 3 from the base chain: no longer
        d.X[2 * c.n - 1, 3] += d.X.dtype.type(2.0 ** -scale_exponents(c.n)[1])
        d.S[:, 2 * c.n - 1] += np.rint(d.A[:, 3] * 2.0 ** scale_exponents(c.n)[0]).astype(np.int64)
    return d


def is_small(c):
    """cells the real-valued tier and the unchanged-inputs check take (a long-double GEMM on the host)"""
    return c.m * c.n * max(c.p, 1) <= 1_500_000


# ------------------------------------------------------------------------------------------------------------ planted mistakes
def restated(d, op, T, base=False, mistake=None, order="forward"):
    """A numpy restatement of an entry on Data d with tanh T (an array function), for the coverage test: the output layout()
    gives for the right kernel, or with ONE mistake planted. order: the summation order of a . x ('forward', 'backward',
    'pairs'), which exact data must not feel."""
    A, X, b = d.A.astype(np.float64), d.X.astype(np.float64), d.b.astype(np.float64)
    m, n = A.shape
    cols = list(range(n))
    if order == "backward":
        cols = cols[::-1]
    elif order == "pairs":
        cols = cols[0::2] + cols[1::2]
    if mistake == "last-pair-dropped":
        cols = [j for j in cols if j < n - 2]
    Ax = A
    if mistake == "k-permutation-on-A-only":
        perm = np.arange(n)
        perm[:2] = perm[:2][::-1]
        Ax = A[:, perm]
    s = np.zeros((m, X.shape[0]))
    for j in cols:
        s = s + Ax[:, j, None] * X[None, :, j]
    t = T(s)
    if mistake == "nan-to-one":
        t = np.where(np.isnan(t), 1.0, t)
    y = t - (np.roll(b, 1) if mistake == "b-of-wrong-row" else b)[:, None]
    if op == "fbd":
        pairs = y[:, :-1] if base else y
        dd = pairs[:, 1::2] - pairs[:, 0::2] if mistake == "pair-sign-reversed" else pairs[:, 0::2] - pairs[:, 1::2]
        if base:
            last = y[:, -2] if mistake == "base-from-point-2n-1" else y[:, -1]
            return np.concatenate([dd.ravel(), last])
        return dd.ravel()
    if mistake == "transposed-store":
        return layout(y, "fbr" if op == "fb" else "fb")
    return layout(y, op)


# ------------------------------------------------------------------------------------------------------------ Gaussian sum, decay
def gauss_blocks(count):
    """workgroups of 256 threads the Gaussian-sum and decay entries launch for `count` outputs (blocks_for, workloads.hip)"""
    return min(max((count + 255) // 256, 1), 2048)


GAUSS_K = (1, 5, 16, 17)
GAUSS_M = (1, 255, 256, 257, 70000)
KGAUSSMAX = 16


def gauss_inputs(m, K, p, dtype=np.float64, seed=0):
    """t, data (m), X (p x (3K + 1)): amplitudes, centres, widths, offset; the last point has one width so small that its exponential
    underflows to zero for every row and (K > 1) one centre far away"""
    rng = np.random.default_rng([seed, m, K, p, 5])
    t = np.sort(rng.uniform(0, 1, m)).astype(dtype)
    data = rng.standard_normal(m).astype(dtype)
    X = np.empty((p, 3 * K + 1))
    X[:, :K] = rng.uniform(0.3, 1.0, (p, K))
    X[:, K:2 * K] = rng.uniform(0, 1, (p, K)) + 1.0 / 3        # (never a t: no 0 * inf)
    X[:, 2 * K:3 * K] = rng.uniform(0.05, 0.3, (p, K))
    X[:, 3 * K] = rng.uniform(-0.2, 0.2, p)
    X[-1, 2 * K] = 1e-3
    X[-1, K] = 2.0                                              # at least 1 from every t: the argument is below -5e5
    if K > 1:
        X[-1, K + 1] = 1e6
    return t, data, X.astype(dtype)


def gauss_arguments(t, x, K):
    """the arguments of the exponentials of one point, one IEEE operation at a time as gauss_g / gauss_row write them:
    g = -1 / ((2 w) w), d = t - c, (d d) g -- m x K, in t's type"""
    dt = t.dtype.type
    w = x[2 * K:3 * K]
    g = (dt(-1) / ((dt(2) * w).astype(t.dtype) * w).astype(t.dtype)).astype(t.dtype)
    d = (t[:, None] - x[None, K:2 * K]).astype(t.dtype)
    return ((d * d).astype(t.dtype) * g[None, :]).astype(t.dtype)


def gauss_reference(t, data, x, K, E, rows=None, mistake=None):
    """y of one point for the rows `rows` (all when None): s = b; s = fma(a_k, E[i, k], s), k ascending; y = fl(s - data).
    E: the device's exponentials of gauss_arguments (m x K)."""
    dt = t.dtype.type
    rows = range(len(t)) if rows is None else rows
    out = np.empty(len(rows), dtype=t.dtype)
    for q, i in enumerate(rows):
        s = x[3 * K]
        for k in range(K):
            s = fma_exact(x[k], E[i, k], s, dt)
        out[q] = dt(s) - data[i]
    return out


def exp_decay_reference(t, data, x, kind, E):
    """(reference in long double, bound) around the device's exponential E of the argument u (exp_decay_argument):
    kind 0: x0 E - data: the product and the subtraction round (one rounding when they are fused): u_T (|x0 E| + |y|);
    kind 1: x0 E + x2 - data: product, addition, subtraction: u_T (|x0 E| + |x0 E + x2| + |y|).
    Each rounding is at most u_T times the EXACT value it rounds; the later ones round values that carry the earlier errors, a
    second-order term this first-order sum leaves out: the bound is widened by the factor 1 + 4 u_T for it."""
    ut = 2.0 ** -53 if t.dtype == np.float64 else 2.0 ** -24
    pe = LD(x[0]) * E.astype(LD)
    if kind == 0:
        y = pe - data.astype(LD)
        return y, ut * (1 + 4 * ut) * (np.abs(pe) + np.abs(y))
    z = pe + LD(x[2])
    y = z - data.astype(LD)
    return y, ut * (1 + 4 * ut) * (np.abs(pe) + np.abs(z) + np.abs(y))


def exp_decay_argument(t, x, kind):
    return ((-t) * x[1]).astype(t.dtype) if kind == 0 else ((-t) / x[1]).astype(t.dtype)
