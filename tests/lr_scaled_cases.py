"""Cases of the SCALED Broyden sweep and flush (csrc/broyden_lr.h: the instances of k_broyden_lr / k_lr_flush that read the unscaled
finite-difference difference panel D and its interval widths twh instead of J; unit entries mir_lsq_lr_pass_scaled_d and
mir_lsq_lr_flush_scaled_d), shared by tests/test_lr_scaled_cell_coverage.py (CPU: the cell list reaches every scaled instance)
and tests/test_gpu_lr_scaled.py (device: every comparison bitwise).

The statement under test: a sweep that loads D[i][j] and forms  twh[j] == 0 ? 0 : D[i][j] * (1 / twh[j])  holds the value the
plain sweep loads from the J that the fused FD kernel (mir_lsq_fd_diff_jtj_d) writes from the same D and twh, so every output of
a pass -- the partial vectors, the reduced vector, column k of U, and behind them JJ, Jy, D[k], the sums -- has the same bits, and
so has the flushed J. The reference J is that kernel's output wherever it covers the shape (n <= 128, n = 192, n = 256); n = 130
has no fused FD kernel, there J is the same expression in numpy (IEEE division and multiplication, correctly rounded on both
sides; test_gpu_lr_scaled also holds the kernel's J to that expression at every n it covers).

twh has zeros in the first, the last and an interior column. D carries a NaN and an Inf in a collapsed column (they must read as
0) in every case, and in the `poisoned` cases also in a live column (they must propagate identically)."""
import collections

import numpy as np

from mir_optim_amd import api
import jtj_cases as JC
from jtj_cases import Guarded, bits
import lr_cases as LC
from lm_solve_cases import named

NS = (1, 7, 32, 33, 64, 100, 127, 128, 130, 192, 256)    # every NCP (1, 2, 4, 8); odd n and the shifted views: the element-wise flavour
MS = (1, 3, 5, 129, 1031)                                # below one 4-row group, ragged groups, two workgroups (1031: 9 groups a wave)
SWEEP_KS = (0, 1, 5, 15)
FLUSH_KS = (1, 2, 16)
SPEC_K = 5                                               # the go and the no-go record run with five pending terms
GO, NOGO = "go", "qp_status"
FD_DIFF_COVERED = tuple(n for n in NS if n <= 128 or n in (192, 256))

Cell = collections.namedtuple("Cell", "kind m n k off mode poisoned")


def collapsed_columns(n):
    return sorted({0, n - 1, n // 2})


def has_live_column(n):
    return len(collapsed_columns(n)) < n


def offsets(n):
    """0: the panel on the 16-byte grid; 1 (even n only): an element-offset view, which takes an even n to the element-wise flavour"""
    return (0, 1) if n % 2 == 0 else (0,)


def _cells():
    c = []
    for n in NS:
        for off in offsets(n):
            for m in MS:
                c += [Cell("pass", m, n, k, off, "plain", False) for k in SWEEP_KS]
                if has_live_column(n):                   # (n = 1: its only column is collapsed)
                    c += [Cell("pass", m, n, 1, off, "plain", True)]
                c += [Cell("pass", m, n, SPEC_K, off, GO, False), Cell("pass", m, n, SPEC_K, off, NOGO, False)]
                c += [Cell("flush", m, n, k, off, "", False) for k in FLUSH_KS]
    assert len(set(c)) == len(c)
    return tuple(c)


CELLS = _cells()


def cell_class(c):
    """the scaled instance a cell runs, through the library's own class function (host code): (kernel, NCP, VEC)"""
    return ("sweep" if c.kind == "pass" else "flush",) + api.lr_class(8, c.n, aligned=(c.off == 0))


# every scaled instance launch_broyden.hip compiles (f64, n <= 256), written out by hand
LISTED = {(kern, ncp, vec) for kern in ("sweep", "flush") for ncp in (1, 2, 4, 8) for vec in (False, True)}


# ---------------------------------------------------------------- data

def panel_case(m, n, poisoned):
    """(D, twh): differences of the size a step of 1e-6 gives, widths near 2e-6 with three zeros; the special values"""
    rng = JC._seed(24, m, n, int(poisoned))
    D = 1e-6 * rng.standard_normal((m, n))
    twh = 2e-6 * (1.0 + 0.25 * rng.random(n))
    zc = collapsed_columns(n)
    twh[zc] = 0.0
    D[0, zc[0]] = np.nan                                  # collapsed: must read as 0
    D[m // 2, zc[-1]] = np.inf
    live = [j for j in range(n) if j not in zc]
    if poisoned:
        assert live, "no live column to poison"
        D[0, live[0]] = np.nan                            # live: must propagate identically
        D[m - 1, live[-1]] = -np.inf
    return D, twh


def scale_by_hand(D, twh):
    """t == 0 ? 0 : d * (1 / t), one reciprocal per column and one multiplication per element"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(twh == 0, 0.0, 1.0 / np.where(twh == 0, 1.0, twh))
        return np.where(inv[None, :] == 0, 0.0, D * inv[None, :])


def reference_J(D, twh, y, off):
    """the J the plain kernels are given: what mir_lsq_fd_diff_jtj_d writes from (D, twh) -- the panel and J shifted like the cell's
    view --, asserted equal to scale_by_hand bit for bit; where no fused FD kernel covers n, scale_by_hand itself"""
    m, n = D.shape
    byhand = scale_by_hand(D, twh)
    if n not in FD_DIFF_COVERED:
        return byhand
    J, _, _ = JC.run_fd_jtj(D, twh, y, True, j_offset_elems=off, jout_offset_elems=off)
    named("reference", np.array_equal(bits(J), bits(byhand)), "the fused FD kernel's J is not d * (1 / twh) at", np.argwhere(bits(J) != bits(byhand))[:4].tolist())
    return J


def pass_inputs(m, n, k, seed=0):
    """U, D (pending steps), y, y_old, JJ, dx, dx_dot of lr_cases.random_inputs; its J is dropped"""
    inp = LC.random_inputs(m, n, k, np.float64, seed=seed)
    inp.pop("J")
    return inp


# ---------------------------------------------------------------- the device
def run_pass_scaled(cell, panel, twh, inp):
    """one mir_lsq_lr_pass_scaled_d on guarded buffers, the panel in J's place and NO J allocated; lr_cases.run_pass's invariants
    plus: the panel and twh come back bit-identical"""
    dt = np.dtype(np.float64)
    m, n = panel.shape
    k = inp["U"].shape[0]
    count = inp["y"].shape[0]
    spec = None if cell.mode == "plain" else LC.spec_of(cell.mode, dt)
    go = spec is None or LC.spec_go_by_hand(*spec)
    gP, gt = Guarded(dt, m * n, panel, cell.off), Guarded(dt, n, twh)
    gU, gD = LC._partial(dt, (k + 1) * m, inp["U"]), LC._partial(dt, (k + 1) * n, inp["D"])
    gdx, gdd = Guarded(dt, n, inp["dx"]), Guarded(dt, 1, inp["dx_dot"])
    gy, gyo = Guarded(dt, count * m, inp["y"]), Guarded(dt, m, inp["y_old"])
    gJJ, gJy = Guarded(dt, n * n, inp["JJ"]), Guarded(dt, n)
    kw = {} if spec is None else dict(spec=spec[0], absTolerance=spec[1], relTolerance=spec[2])
    r = api.lrPass(m, n, k, gP.ptr, gU.ptr, gD.ptr, gdx.ptr, gdd.ptr, gy.ptr, gyo.ptr, gJJ.ptr, gJy.ptr, dtype=dt, count=count, twh=gt.ptr, **kw)
    fin = spec is None
    out = {key: g.finish(key, w) for key, g, w in (("panel", gP, False), ("twh", gt, False), ("U", gU, go), ("D", gD, fin), ("dx", gdx, False),
                                                   ("dx_dot", gdd, False), ("y", gy, False), ("y_old", gyo, False), ("JJ", gJJ, fin), ("Jy", gJy, fin))}
    named("invariants", r["guard"] == -1 and r["bands"] == 7, "guard band", r["guard"], "of", r["bands"])
    named("invariants", r["touched"] == 0, "state / record written", r["touched"])
    named("invariants", ("sweep",) + r["cls"] == cell_class(cell), r["cls"])
    Uo, Do = out["U"].reshape(k + 1, m), out["D"].reshape(k + 1, n)
    named("invariants", np.array_equal(bits(Uo[:k]), bits(inp["U"])), "a column < k of U changed")
    named("invariants", np.array_equal(bits(Do[:k]), bits(inp["D"])), "a row < k of D changed")
    r.update(U_col=Uo[k], D=Do, JJ=out["JJ"].reshape(n, n), Jy=out["Jy"])
    return r


def run_flush_scaled(cell, panel, twh, inp):
    """one mir_lsq_lr_flush_scaled_d: J a guarded OUTPUT (the guard pattern until written), the panel, twh, U, D read-only between
    their bands; -> the materialised J"""
    dt = np.dtype(np.float64)
    m, n = panel.shape
    k = inp["U"].shape[0]
    gJ = Guarded(dt, m * n, None, cell.off)
    gP, gt = Guarded(dt, m * n, panel, cell.off), Guarded(dt, n, twh)
    gU, gD = Guarded(dt, k * m, inp["U"]), Guarded(dt, k * n, inp["D"])
    cls = api.lrFlushScaled(m, n, k, gJ.ptr, gP.ptr, gt.ptr, gU.ptr, gD.ptr)
    out = {key: g.finish(key, w) for key, g, w in (("J", gJ, True), ("panel", gP, False), ("twh", gt, False), ("U", gU, False), ("D", gD, False))}
    named("invariants", ("flush",) + cls == cell_class(cell), cls)
    return out["J"].reshape(m, n)


PASS_KEYS = ("reduced", "U_col", "partials", "sums")
FINISH_KEYS = ("JJ", "Jy", "D")


def check_same_pass(scaled, plain, finished):
    """every output of the scaled pass against the plain pass on the reference J, bit for bit (NaNs included)"""
    for key in PASS_KEYS + (FINISH_KEYS if finished else ()):
        a, b = np.asarray(scaled[key]), np.asarray(plain[key])
        named("scaled", a.shape == b.shape and np.array_equal(bits(a), bits(b)), key, "differs at", np.argwhere(bits(a) != bits(b))[:6].tolist() if a.shape == b.shape else (a.shape, b.shape))
    if finished:
        named("scaled", bits(np.array([scaled["jy_inf"]]))[0] == bits(np.array([plain["jy_inf"]]))[0], "jy_inf", scaled["jy_inf"], plain["jy_inf"])
    named("scaled", scaled["nblk"] == plain["nblk"], "workgroups", scaled["nblk"], plain["nblk"])
