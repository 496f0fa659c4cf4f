"""Kernel-level cases of the J^T J kernels (csrc/jtj_plan.h): one guarded runner over the unit entries mir_lsq_jtj_* /
mir_lsq_fd_jtj_d / mir_lsq_fd_diff_jtj_d, plain numpy references with derived error bounds, exact-integer generators, the
list CELLS of shapes the GPU file runs and the universe INSTANTIATED of kernel instances launch_jtj.hip compiles.
No GPU is needed to import this module; only run_jtj / run_fd_jtj touch one. LS = least_squares.d of the reference."""
import ctypes as C

import numpy as np

from mir_optim_amd import api

# ---- guard bands ---------------------------------------------------------------------------------------------------------
GUARD_BYTES = 4096                       # in front of and behind every payload: a multiple of 256, at least 4 KiB
NAN_BITS = {4: 0x7FC5A5A5, 8: 0x7FF85A5A5A5A5A5A}      # one quiet NaN per element size; guards are compared as unsigned integers
UINT = {4: np.uint32, 8: np.uint64}


class Guarded:
    """A device array between two guard bands. Everything in the allocation that is not payload holds NAN_BITS -- the front
    band, the `offset_elems` elements that shift the payload off the 16-byte grid, the round-up to 256 bytes and the back band --
    and so does the payload of an output until a kernel writes it."""

    def __init__(self, dtype, count, payload=None, offset_elems=0):
        self.dtype = np.dtype(dtype)
        es = self.dtype.itemsize
        assert GUARD_BYTES % 256 == 0 and GUARD_BYTES >= 4096 and offset_elems in (0, 1)
        self.count = int(count)
        self.start = GUARD_BYTES // es + offset_elems                       # first payload element
        body = -(-((offset_elems + self.count) * es) // 256) * 256
        self.total = (GUARD_BYTES + body + GUARD_BYTES) // es
        self.image = np.full(self.total, NAN_BITS[es], dtype=UINT[es])
        self.buf = api.DeviceBuffer(self.image)
        if payload is not None:
            payload = np.ascontiguousarray(payload, dtype=self.dtype).reshape(-1)
            assert payload.size == self.count
            self.buf.upload_at(self.start * es, payload.view(UINT[es]))
            self.image[self.start:self.start + self.count] = payload.view(UINT[es])
        self.ptr = self.buf.ptr + self.start * es
        assert self.ptr % 16 == (offset_elems * es) % 16

    def finish(self, name, written):
        """download the whole buffer, free it, assert every guard word (written=False: every word) bit-identical; -> payload"""
        got = self.buf.download()
        self.buf.free()
        lo, hi = self.start, self.start + self.count
        for part, a, b in (("front guard", 0, lo), ("back guard", hi, self.total)) + (() if written else (("read-only payload", lo, hi),)):
            bad = np.flatnonzero(got[a:b] != self.image[a:b])
            assert bad.size == 0, f"{name}: {bad.size} words of the {part} changed, first at element {a + int(bad[0]) - lo} relative to the payload"
        return got[lo:hi].view(self.dtype).copy()


def run_jtj(J, y, y_old=None, dx=None, dtype=np.float64, j_offset_elems=0):
    """mir_lsq_jtj_d / _s on guarded buffers; with dx: the Broyden rewrite. Only J may be shifted (by one element: 8 mod 16 bytes
    for f64, 4 mod 16 for f32); y, y_old, dx keep the alignment they have in the solver. -> (JJ, Jy, J_after)"""
    dtype = np.dtype(dtype)
    J = np.ascontiguousarray(J, dtype=dtype)
    m, n = J.shape
    broyden = dx is not None
    gJ = Guarded(dtype, m * n, J, j_offset_elems)
    gy = Guarded(dtype, m, y)
    gyo = Guarded(dtype, m, y_old if broyden else y)
    gdx = Guarded(dtype, n, dx if broyden else np.zeros(n))
    gJJ, gJy = Guarded(dtype, n * n), Guarded(dtype, n)
    fn = api.lib().mir_lsq_jtj_d if dtype == np.float64 else api.lib().mir_lsq_jtj_s
    rc = fn(m, n, gJ.ptr, gy.ptr, gyo.ptr, gdx.ptr, 1 if broyden else 0, gJJ.ptr, gJy.ptr, None, C.byref(C.c_float(0)))
    out = {k: g.finish(k, w) for k, g, w in (("J", gJ, broyden), ("y", gy, False), ("y_old", gyo, False), ("dx", gdx, False),
                                             ("JJ", gJJ, True), ("Jy", gJy, True))}
    assert rc == 0, f"mir_lsq_jtj: {rc}"
    return out["JJ"].reshape(n, n), out["Jy"], out["J"].reshape(m, n)


def run_fd_jtj(panel, twh, y, diff, j_offset_elems=0, jout_offset_elems=0, keep=False):
    """mir_lsq_fd_jtj_d (panel: m x 2n pairs) / mir_lsq_fd_diff_jtj_d (diff: the m x n difference panel) on guarded buffers.
    The difference panel and Jout may be shifted independently; the pair panel is the library's own buffer in the solver and
    jtj_resolve does not reroute it, so it stays aligned. keep (fd_diff_keep): the call is made with J = NULL and the J buffer,
    which no kernel is given, must come back untouched. -> (J, JJ, Jy); keep: (the panel as it came back, JJ, Jy)"""
    panel = np.ascontiguousarray(panel, dtype=np.float64)
    m, n = panel.shape[0], panel.shape[1] if diff else panel.shape[1] // 2
    assert diff or j_offset_elems == 0
    gP = Guarded(np.float64, panel.size, panel, j_offset_elems)
    gt, gy = Guarded(np.float64, n, twh), Guarded(np.float64, m, y)
    gJ = Guarded(np.float64, m * n, None, jout_offset_elems)
    gJJ, gJy = Guarded(np.float64, n * n), Guarded(np.float64, n)
    L = api.lib()
    assert diff or not keep
    rc = (L.mir_lsq_fd_diff_jtj_d if diff else L.mir_lsq_fd_jtj_d)(m, n, gP.ptr, gt.ptr, gy.ptr, None if keep else gJ.ptr, gJJ.ptr, gJy.ptr,
                                                                 None, None)
    out = {k: g.finish(k, w) for k, g, w in (("panel", gP, False), ("twh", gt, False), ("y", gy, False), ("Jout", gJ, not keep),
                                             ("JJ", gJJ, True), ("Jy", gJy, True))}
    assert rc == 0, f"mir_lsq_fd_jtj: {rc}"
    return out["panel" if keep else "Jout"].reshape(m, n), out["JJ"].reshape(n, n), out["Jy"]


# ---- references and bounds -----------------------------------------------------------------------------------------------
UNIT = {4: 2.0 ** -24, 8: 2.0 ** -53}                                   # unit roundoff of the kernels' type
REF_UNIT = {4: 2.0 ** -53, 8: float(np.finfo(np.longdouble).eps) / 2}   # ... and of the type the reference sums in


def gamma(k, u):
    assert k * u < 0.01
    return k * u / (1 - k * u)


def _wide(dtype):
    return np.longdouble if np.dtype(dtype) == np.float64 else np.float64


def ref_products(J, y):
    """J^T J and J^T y of J as given (LS:1065, 1052), formed in longdouble for f64 inputs and in float64 for f32 inputs"""
    W = _wide(J.dtype)
    Jt = np.ascontiguousarray(J.astype(W).T)
    n, B = J.shape[1], 32
    JJ = np.empty((n, n), dtype=W)
    # numpy has no BLAS for longdouble: the lower triangle of 32-column blocks from contiguous rows of J^T, mirrored (each entry is
    # the same sum of the same commuting products on both sides); about four times faster at n = 256 than J^T J in one call
    for i in range(0, n, B):
        for j in range(0, i + 1, B):
            blk = Jt[i:i + B] @ Jt[j:j + B].T
            JJ[i:i + B, j:j + B] = blk
            JJ[j:j + B, i:i + B] = blk.T
    return JJ, Jt @ np.asarray(y).astype(W)


def product_bound(J, y, dtype):
    """Elementwise bound on |computed - ref_products| for ANY summation order, FMA or not: a length-m inner product computed
    with unit roundoff u satisfies |fl(a.b) - a.b| <= gamma_m |a|.|b| (every term passes through at most one multiplication and
    m - 1 additions; Higham, Accuracy and Stability, section 3.1). The reference is itself a computed inner product in a wider type:
    its gamma_m is added. |J|^T |J| itself is summed in float64, all terms positive, so the true sum is at most the computed one
    times 1 + gamma_{m+1}(2^-53). Derived, not measured."""
    es = np.dtype(dtype).itemsize
    m = J.shape[0]
    g = (gamma(m, UNIT[es]) + gamma(m, REF_UNIT[es])) * (1 + gamma(m + 1, 2.0 ** -53))
    A = np.abs(J.astype(np.float64))
    return g * (A.T @ A), g * (A.T @ np.abs(np.asarray(y).astype(np.float64)))


def broyden_reference(J, y, y_old, dx):
    """LS:1002-1006 in the wider type, and an elementwise bound on |J_after - reference| for a kernel that works in J.dtype.
      d = 1 / (dx.dx);  u_i = -d ((y_old_i - y_i) + J_i.dx);  J_after_ij = J_ij + u_i dx_j
    Rounding model (u = unit roundoff, every operation rounded once, sums in any order):
      computed d = d (1 + th), |th| <= gamma_{n+1}: n positive terms and one division;
      computed t_i = fl(fl(y_old_i - y_i) + fl(J_i.dx)): |err| <= gamma_{n+2} (|y_old_i| + |y_i| + |J_i|.|dx|);
      computed u_i = fl(-d^ t^_i): |err| <= E_i = |d| gamma_{n+2} (|y_old_i| + |y_i| + |J_i|.|dx|) + gamma_{n+3} |u_i|  (first order);
      computed J_after_ij = fl(J_ij + fl(u^_i dx_j)): |err| <= u |J_ij + u_i dx_j| + |dx_j| (E_i + u |u_i|)
                                                           <= u |J_ij| + |dx_j| (E_i + 2 u |u_i|)            (first order).
    The returned bound is twice that: the factor 2 covers every second-order term (all gammas here are below 1e-2)."""
    es = J.dtype.itemsize
    W, u, n = _wide(J.dtype), UNIT[es], J.shape[1]
    Jw, yw, yow, dxw = (np.asarray(a).astype(W) for a in (J, y, y_old, dx))
    d = 1 / (dxw @ dxw)
    ui = -d * ((yow - yw) + Jw @ dxw)
    ref = Jw + np.outer(ui, dxw)
    E = abs(d) * gamma(n + 2, u) * (np.abs(yow) + np.abs(yw) + np.abs(Jw) @ np.abs(dxw)) + gamma(n + 3, u) * np.abs(ui)
    bound = 2 * (u * np.abs(Jw) + np.outer(E + 2 * u * np.abs(ui), np.abs(dxw)))
    return ref, bound


def ref_fill(panel, twh, diff):
    """LS:1041-1047 in the reference's operation order: copy, axpy(-1), scal(1 / twh); a collapsed interval gives a zero column"""
    if diff:
        d = np.array(panel, dtype=np.float64)
    else:
        d = panel[:, 0::2].copy()
        d += -1.0 * panel[:, 1::2]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / twh
        J = d * inv
    J[:, twh == 0] = 0.0
    return J


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def same_bits(a, b):
    """bit for bit, NaNs included; only the sign of a zero is left open (x + 0 turns -0 into +0 and changes nothing else): an exactly
    cancelling sum is +0 or -0 by the order of its terms, which no reference fixes"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a + 0), bits(b + 0))


# ---- generators ------------------------------------------------------------------------------------------------------------
def _seed(*k):
    return np.random.default_rng([abs(int(v)) for v in k])


def asym_col(n):
    return 1 if n > 1 else 0


def exact_dx(n):
    """four entries +-0.5 (n >= 4), two (n = 2, 3), one entry +-1 (n = 1): dx.dx is a power of two"""
    dx = np.zeros(n)
    if n == 1:
        dx[0] = -1.0
    elif n < 4:
        dx[0], dx[n - 1] = 0.5, -0.5
    else:
        dx[[0, n // 3, (2 * n) // 3, n - 1]] = (0.5, -0.5, 0.5, -0.5)
    return dx


def assert_exact_precondition(JJr, Jyr):
    """every partial sum of the products is a multiple of 1/16 (1/4) below 2^24 in magnitude: exact in f32 and f64, any order"""
    assert 16 * float(np.abs(JJr).max()) < 2 ** 24 and 4 * float(np.abs(Jyr).max()) < 2 ** 24


def exact_case(m, n, dtype, rewrite):
    """integers in [-3, 3], one asymmetric column (a transposed accumulator map changes J^T J); rewrite: d, t, u exact, J_after a
    multiple of 1/4. -> dict(J, y, y_old, dx, J_after, JJ, Jy), all exact in `dtype`"""
    rng = _seed(1, m, n, rewrite)
    J = rng.integers(-3, 4, size=(m, n)).astype(dtype)
    J[:, asym_col(n)] = (np.arange(m) % 5 - 2).astype(dtype)
    y = rng.integers(-3, 4, size=m).astype(dtype)
    y_old = rng.integers(-3, 4, size=m).astype(dtype)
    c = dict(J=J, y=y, y_old=None, dx=None, J_after=J)
    if rewrite:
        dx = exact_dx(n).astype(dtype)
        ref, _ = broyden_reference(J, y, y_old, dx)
        Ja = ref.astype(dtype)
        assert np.array_equal(Ja.astype(ref.dtype), ref) and np.array_equal(4 * ref, np.rint(4 * ref))
        c.update(y_old=y_old, dx=dx, J_after=Ja)
    JJr, Jyr = ref_products(c["J_after"], y)
    assert_exact_precondition(JJr, Jyr)
    c.update(JJ=JJr.astype(dtype), Jy=Jyr.astype(dtype))
    return c


def random_case(m, n, dtype, rewrite):
    rng = _seed(2, m, n, rewrite)
    J = rng.standard_normal((m, n)).astype(dtype)
    J[:, asym_col(n)] = (np.arange(m) % 5 - 2).astype(dtype)
    y_old = rng.standard_normal(m).astype(dtype)
    y = (y_old + 0.1 * rng.standard_normal(m)).astype(dtype)
    dx = (0.05 * rng.standard_normal(n)).astype(dtype)
    return dict(J=J, y=y, y_old=y_old if rewrite else None, dx=dx if rewrite else None)


def fd_case(m, n, diff, exact):
    """pair panel (or its difference), interval widths with a clipped and -- n > 3 -- a collapsed interval, y, and the Jacobian
    of ref_fill; exact: integers in [-3, 3] and widths 2 and 1, so J is a multiple of 1/2 in [-6, 6]"""
    rng = _seed(3, m, n, diff, exact)
    if exact:
        Y = rng.integers(-3, 4, size=(m, 2 * n)).astype(np.float64)
        Y[:, 2 * asym_col(n)] = np.arange(m) % 5 - 2.0
        twh = np.full(n, 2.0)
        twh[n // 2] = 1.0
        y = rng.integers(-3, 4, size=m).astype(np.float64)
    else:
        base, Jt, h = rng.standard_normal((m, 1)), rng.standard_normal((m, n)), 2.0 ** -26
        Y = np.empty((m, 2 * n))
        Y[:, 0::2], Y[:, 1::2] = base + h * Jt, base - h * Jt
        twh = np.full(n, 2 * h)
        twh[n // 2] = h
        y = rng.standard_normal(m)
    if n > 3:
        twh[3] = 0.0
    J = ref_fill(Y, twh, False)
    panel = Y
    if diff:
        panel = Y[:, 0::2].copy()
        panel += -1.0 * Y[:, 1::2]                          # LS:1041, 1045 done by the caller
        assert np.array_equal(ref_fill(panel, twh, True), J)
    c = dict(panel=panel, twh=twh, y=y, J=J)
    if exact:
        JJr, Jyr = ref_products(J, y)
        assert_exact_precondition(JJr, Jyr)
        c.update(JJ=JJr.astype(np.float64), Jy=Jyr.astype(np.float64))
    return c


# ---- the shapes the GPU file runs: (elem_size, op, m, n, j_offset_elems) -------------------------------------------------------
M_ODD, M_EVEN = 1001, 1002               # several workgroups of 128 to 256 rows with a partial last one
SMALL_MS = (1, 3, 67)                    # below one 4-row group, below one stage, a partial stage (67 % 4 == 3)


def _cells():
    c = []
    for k in range(1, 9):                # n <= 128: one n on the 16-column grid and at least one off it per block count
        on, odd, even, quad = 16 * k, 16 * k - 3, 16 * k - 6, 16 * k - 4
        c += [(8, "rewrite", M_ODD, on, 0), (8, "rewrite", M_ODD, odd, 0)]                               # stream, f64 rewrite
        c += [(4, "rewrite", M_ODD, on, 0), (4, "rewrite", M_ODD, odd, 0)]                               # stream, f32 rewrite
        c += [(4, "plain", M_ODD, odd, 0), (4, "plain", M_EVEN, even, 0)]                                # stream, f32 plain (n % 4 != 0)
        c += [(4, "plain", M_ODD, on, 0), (4, "plain", M_ODD, quad, 0)]                                  # pc32 (n % 4 == 0)
        c += [(8, "plain", M_EVEN, on, 0), (8, "plain", M_ODD, even, 0), (8, "plain", M_ODD, odd, 0)]    # fdp plain; odd n: flat
        c += [(8, "fd", M_EVEN, on, 0), (8, "fd", M_ODD, odd, 0)]                                        # fdp fd
        c += [(8, "fd_diff", M_EVEN, on, 0), (8, "fd_diff", M_ODD, on, 0)]                               # fdp fd_diff
        c += [(8, "fd_diff", M_ODD, odd, 0), (8, "fd_diff", M_EVEN, even, 0)]                            # ... flat (n % 16 != 0)
        c += [(8, "fd_diff_keep", M_EVEN, on, 0), (8, "fd_diff_keep", M_ODD, on, 0)]                     # fdp_nw
        c += [(8, "fd_diff_keep", M_ODD, odd, 0), (8, "fd_diff_keep", M_EVEN, even, 0)]                  # fdp flat with a null Jout
    for k in range(9, 17):               # ring8: n % 16 == 0 and even m
        c += [(8, "plain", M_EVEN, 16 * k, 0), (8, "rewrite", M_EVEN, 16 * k, 0)]
    for n in (160, 192, 224, 256):       # fdp8 at 10, 12, 14, 16 blocks: on the grid (plain: odd m) and off it (padding columns)
        c += [(8, "plain", M_ODD, n, 0), (8, "plain", M_ODD, n - 3, 0), (8, "plain", M_EVEN, n - 24, 0)]
        c += [(8, "fd", M_EVEN, n, 0), (8, "fd", M_ODD, n - 3, 0), (8, "fd", M_ODD, n - 24, 0)]
    c += [(8, op, m, n, 0) for op in ("fd_diff", "fd_diff_keep") for n in (192, 256) for m in (M_ODD, M_EVEN)]
    # wide: every tile grid here has an off-diagonal job
    c += [(4, op, M_ODD, n, 0) for op in ("plain", "rewrite") for n in (129, 200, 256, 300)]
    c += [(8, "plain", M_ODD, 300, 0), (8, "plain", M_EVEN, 257, 0)]
    c += [(8, "rewrite", M_ODD, 200, 0), (8, "rewrite", M_ODD, 300, 0), (8, "rewrite", M_ODD, 256, 0)]
    # per family and type, once each: the small row counts (ring8 takes even m only: 2, 66)
    for m in SMALL_MS:
        c += [(8, "rewrite", m, 77, 0), (4, "rewrite", m, 100, 0), (4, "plain", m, 90, 0), (4, "plain", m, 64, 0)]
        c += [(8, "plain", m, 64, 0), (8, "plain", m, 33, 0), (8, "fd", m, 48, 0), (8, "fd_diff", m, 64, 0), (8, "fd_diff", m, 33, 0)]
        c += [(8, "plain", m, 200, 0), (8, "fd", m, 200, 0), (8, "fd_diff", m, 192, 0)]
        c += [(8, "fd_diff_keep", m, 64, 0), (8, "fd_diff_keep", m, 33, 0), (8, "fd_diff_keep", m, 192, 0)]
        c += [(4, "plain", m, 200, 0), (4, "rewrite", m, 200, 0), (4, "rewrite", m, 300, 0), (8, "plain", m, 300, 0),
              (8, "rewrite", m, 200, 0), (8, "rewrite", m, 300, 0)]
    c += [(8, op, m, 144, 0) for op in ("plain", "rewrite") for m in (2, 66)]
    # J one element off the 16-byte grid
    c += [(4, "plain", M_ODD, n, 1) for n in (64, 100, 128)]                  # pc32 -> stream
    c += [(8, "plain", M_EVEN, n, 1) for n in (16, 64, 126, 128)]             # fdp -> flat producer, even n
    c += [(8, op, M_EVEN, n, 1) for op in ("fd_diff", "fd_diff_keep") for n in (64, 128)]   # ... for the difference panel (fdp_nw too)
    c += [(8, "rewrite", M_ODD, 77, 1), (4, "rewrite", M_ODD, 100, 1), (8, "plain", M_ODD, 200, 1),
          (4, "plain", M_ODD, 300, 1), (8, "rewrite", M_ODD, 300, 1)]         # same kernel for both alignments
    assert len(set(c)) == len(c)
    return c


CELLS = _cells()
JOUT_OFFSET_CELLS = [(8, "fd_diff", M_EVEN, 64, 0)]        # run once more with only Jout shifted (consumers' and producers' write-back)
NAN_MS = (66, 67)                                          # NaN localisation: the cells with these row counts, plain and rewrite


def cell_id(cell):
    es, op, m, n, off = cell
    return f"f{8 * es}-{op}-m{m}-n{n}" + ("-offset" if off else "")


# ---- what launch_jtj.hip instantiates, written out independently of jtj_plan<T>() ---------------------------------------
# key: (elem_size, op, family, blocks, flat, pointer). blocks: the NCB template argument; wide is one instance per type, so its
# classes are named instead ("any" / "n<=256" / "n>256": k_broyden_wide or k_broyden_rows in front). pointer: "any", or "offset" for
# a launch that exists only for a J that is not 16-byte aligned (the jtj_resolve outcomes).
RING8_OFFSET = ("unverified_offset: k_jtj8 issues 16-byte global_load_lds from J, y and y_old, jtj_resolve keeps ring8 for an "
                "unaligned J, and nothing in the code establishes that a 16-byte LDS-DMA from an 8-byte-aligned address is defined")


FDP_KEEP_4GB = ("unverified_4gb: fd_diff_keep stays on k_jtj_fdp's strided producer (Jout == nullptr) only where a workgroup's rows span "
                "at least 4 GB of panel; the plan's side of the rule is tests/test_jtj_plan.py's, the kernel is fd_diff's")


def _instantiated():
    u = {}
    for k in range(1, 9):
        for es, op in ((4, "plain"), (4, "rewrite"), (8, "rewrite")):
            u[(es, op, "stream", k, False, "any")] = "run"
        for op, flat in (("fd", False), ("fd_diff", False), ("fd_diff", True), ("plain", False), ("plain", True), ("fd_diff_keep", True)):
            u[(8, op, "fdp", k, flat, "any")] = "run"
        u[(8, "fd_diff_keep", "fdp_nw", k, False, "any")] = "run"
        u[(8, "fd_diff_keep", "fdp", k, False, "any")] = FDP_KEEP_4GB
        u[(4, "plain", "pc32", k, False, "any")] = "run"
    for k in range(9, 17):
        for op in ("plain", "rewrite"):
            u[(8, op, "ring8", k, False, "any")] = "run"
            u[(8, op, "ring8", k, False, "offset")] = RING8_OFFSET
    for k in (10, 12, 14, 16):
        u[(8, "plain", "fdp8", k, False, "any")] = u[(8, "fd", "fdp8", k, False, "any")] = "run"
    for k in (12, 16):
        u[(8, "fd_diff", "fdp8", k, False, "any")] = u[(8, "fd_diff_keep", "fdp8", k, False, "any")] = "run"
    for es in (4, 8):
        for op, cls in (("plain", "any"), ("rewrite", "n<=256"), ("rewrite", "n>256")):
            u[(es, op, "wide", cls, False, "any")] = "run"
    # jtj_resolve: pc32 -> stream with n % 4 == 0 (blocks 4, 7, 8: n = 64, 100, 128); fdp -> flat with even n
    for k in (4, 7, 8):
        u[(4, "plain", "stream", k, False, "offset")] = "run"
    for k in (1, 4, 8):
        u[(8, "plain", "fdp", k, True, "offset")] = "run"
    for k in (4, 8):
        u[(8, "fd_diff", "fdp", k, True, "offset")] = u[(8, "fd_diff_keep", "fdp", k, True, "offset")] = "run"
    return u


INSTANTIATED = _instantiated()


def cell_key(cell, num_cu):
    """the INSTANTIATED key a cell lands on, through the library's own plan (host code)"""
    es, op, m, n, off = cell
    p = api.jtj_plan(es, m, n, num_cu, op, aligned=(off == 0))
    q = api.jtj_plan(es, m, n, num_cu, op, aligned=True)
    fam, blocks = p["family"], p["ncb"]
    if fam == "wide":
        blocks = "any" if op == "plain" else ("n<=256" if n <= 256 else "n>256")
    rerouted = off != 0 and (p["family"], p["flat"]) != (q["family"], q["flat"])
    pointer = "offset" if rerouted or (off != 0 and fam == "ring8") else "any"
    return (es, op, fam, blocks, bool(p["flat"]), pointer), p
