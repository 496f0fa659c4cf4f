"""The store-free instance of the fused FD kernel (csrc/jtj_fdp.h: k_jtj_fdp_nw, the aligned difference panel with J = NULL --
store-free consumers, the lean producer) against the WRITING instance of the same build: mir_lsq_fd_diff_jtj_d with J = NULL and
with a J buffer on the same panel. Every comparison is BITWISE.

  * n = 16, 48, 128 run k_jtj_fdp_nw; n = 100 (padding columns, a row of J off the 128-byte grid), an odd n and an offset view
    run the flat producer of k_jtj_fdp: they must still agree with their J-buffer runs. Which kernel a shape runs is asked of the
    library's plan (operation fd_diff_keep: what the J = NULL call names), not inferred from n.
  * Every shape runs twice: with live columns only (the lean producer's steady state: multiplies and LDS writes alone) and with
    one collapsed column whose panel entries are NaN and Inf (every wave then takes the selects; the column contributes exactly 0).
  * m: around one and two 32-row stages; the smallest even m at which the plan's grid leaves workgroups without a stage; and
    32 g k - 1, 32 g k, 32 g k + 1 for the plan's grid g at m = 32 g k and the smallest k that has such an m (every workgroup
    has exactly k full stages; one row less: the last stage partial; one row more: one more stage, an odd count in the first
    workgroups: the producer's peeled last stage). For odd m the plan takes k_jtj's grid, so the two neighbours also run other
    partitions of the same stages.
  * The panel, twh and y come back unchanged between their guard bands, the NaN bands around JJ and Jy (and J) are intact
    (jtj_cases.Guarded), a second call gives the same bits, and the J of the J-buffer call is lr_scaled_cases.scale_by_hand."""
import ctypes as C
import functools

import numpy as np
import pytest

from mir_optim_amd import api
import jtj_cases as K
from jtj_cases import Guarded, bits
import lr_scaled_cases as S

pytestmark = pytest.mark.gpu

NS = (16, 48, 100, 128)
SMALL_MS = (1, 31, 32, 33, 63, 64, 65)
RS = 32                                                    # rows per stage of k_jtj_fdp's plain layout


@functools.lru_cache(maxsize=None)
def num_cu():
    """the compute units the unit entries plan with: the library's own device query (mirlsq::query_num_cu(), workspace.hip)"""
    f = getattr(api.lib(), "_ZN6mirlsq12query_num_cuEv")
    f.restype, f.argtypes = C.c_int, []
    n = f()
    assert 1 <= n <= 4096, n
    return n


def keep_plan(m, n, aligned=True):
    """what the J = NULL call launches, from the library's plan; the J-buffer call it is compared with runs fd_diff's entry, fdp on
    the same grid, LDS and slabs"""
    p, w = (api.jtj_plan(8, m, n, num_cu(), op, aligned) for op in ("fd_diff_keep", "fd_diff"))
    assert w["family"] == "fdp" and {k: v for k, v in p.items() if k != "family"} == {k: v for k, v in w.items() if k != "family"}, (m, n, p, w)
    return p


def grid(m, n):
    p = keep_plan(m, n)
    # the store-free kernel at n % 16 == 0, else the flat producer of k_jtj_fdp
    assert (p["family"], p["flat"]) == (("fdp_nw", 0) if n % 16 == 0 else ("fdp", 1)), (m, n, p)
    return p["grid"]


def stages_of_last_workgroup(m, n):
    g, stot = grid(m, n), -(-m // RS)
    per = -(-stot // g)
    return max(0, stot - per * (g - 1))


@functools.lru_cache(maxsize=None)
def m_with_idle_workgroups(n):
    """the smallest even m (whole stages plus one) at which the plan's last workgroup gets no stage"""
    for m in range(RS, 400000, RS):
        if grid(m, n) > 1 and stages_of_last_workgroup(m, n) == 0:
            return m
    raise AssertionError(f"no m below 400000 leaves a workgroup of n = {n} without a stage")


@functools.lru_cache(maxsize=None)
def m_of_whole_workgroups(n):
    """m = 32 g k for the smallest k that has one, g >= 2 the plan's grid at that m: every workgroup has exactly k full stages"""
    for k in range(1, 17):
        for g in range(2, 8 * num_cu() + 1):
            if grid(RS * g * k, n) == g:
                return RS * g * k
    raise AssertionError(f"no grid of n = {n} has whole 32-row stages in every workgroup")


def ms_of(n):
    mw = m_of_whole_workgroups(n)
    return tuple(dict.fromkeys(SMALL_MS + (m_with_idle_workgroups(n), mw - 1, mw, mw + 1)))   # (n = 100: mw = 64 is among the small ones)


def panel_case(m, n, collapsed):
    """(D, twh, y, zero column or None): differences of the size a step of 1e-6 gives, widths near 2e-6; collapsed: one zero width,
    with a NaN and an Inf among that column's differences"""
    rng = K._seed(27, m, n, int(collapsed))
    D = 1e-6 * rng.standard_normal((m, n))
    twh = 2e-6 * (1.0 + 0.25 * rng.random(n))
    y = rng.standard_normal(m)
    zc = None
    if collapsed:
        zc = n // 2
        twh[zc] = 0.0
        D[0, zc] = np.nan
        D[m // 2, zc] = np.inf
        D[m - 1, zc] = -np.inf
    return D, twh, y, zc


def run(D, twh, y, write_J, off=0):
    """mir_lsq_fd_diff_jtj_d on guarded buffers (the panel and J shifted by `off` elements); J = NULL unless write_J.
    Guarded.finish asserts the inputs unchanged and every guard word intact. -> (J or None, JJ, Jy)"""
    m, n = D.shape
    gP = Guarded(np.float64, m * n, D, off)
    gt, gy = Guarded(np.float64, n, twh), Guarded(np.float64, m, y)
    gJ = Guarded(np.float64, m * n, None, off) if write_J else None
    gJJ, gJy = Guarded(np.float64, n * n), Guarded(np.float64, n)
    rc = api.lib().mir_lsq_fd_diff_jtj_d(m, n, gP.ptr, gt.ptr, gy.ptr, gJ.ptr if write_J else None, gJJ.ptr, gJy.ptr, None, None)
    for name, g in (("panel", gP), ("twh", gt), ("y", gy)):
        g.finish(name, False)
    J = gJ.finish("J", True).reshape(m, n) if write_J else None
    JJ, Jy = gJJ.finish("JJ", True).reshape(n, n), gJy.finish("Jy", True)
    assert rc == 0, f"mir_lsq_fd_diff_jtj_d: {rc}"
    return J, JJ, Jy


def check_shape(m, n, collapsed, off=0):
    D, twh, y, zc = panel_case(m, n, collapsed)
    J, JJw, Jyw = run(D, twh, y, True, off)
    _, JJ0, Jy0 = run(D, twh, y, False, off)
    _, JJ1, Jy1 = run(D, twh, y, False, off)
    tag = (m, n, collapsed, off)
    assert np.array_equal(bits(JJ0), bits(JJw)), (tag, "JJ", np.argwhere(bits(JJ0) != bits(JJw))[:4].tolist())
    assert np.array_equal(bits(Jy0), bits(Jyw)), (tag, "Jy", np.flatnonzero(bits(Jy0) != bits(Jyw))[:4].tolist())
    assert np.array_equal(bits(JJ1), bits(JJ0)) and np.array_equal(bits(Jy1), bits(Jy0)), (tag, "a second call differs")
    byhand = S.scale_by_hand(D, twh)
    assert np.array_equal(bits(J), bits(byhand)), (tag, "J", np.argwhere(bits(J) != bits(byhand))[:4].tolist())
    assert np.all(np.isfinite(JJ0)) and np.all(np.isfinite(Jy0)), (tag, "a collapsed column's NaN / Inf got through")
    assert np.array_equal(bits(JJ0), bits(np.ascontiguousarray(JJ0.T))), (tag, "JJ is not symmetric")
    if zc is not None:
        zero = bits(np.zeros(1))[0]
        assert np.all(bits(JJ0[zc]) == zero) and np.all(bits(JJ0[:, zc]) == zero) and bits(Jy0[zc:zc + 1])[0] == zero, (tag, "zero column")
    assert np.any(JJ0 != 0), tag


@pytest.mark.parametrize("collapsed", [False, True], ids=["live", "collapsed"])
@pytest.mark.parametrize("n", NS)
def test_null_j_has_the_bits_of_the_writing_instance(n, collapsed):
    for m in ms_of(n):
        check_shape(m, n, collapsed)


def test_the_cases_reach_what_they_are_for():
    """the shapes above on this device's plan: n = 16, 48, 128 run the store-free kernel at every m of the test, n = 100 the flat
    producer; the idle-workgroup shape leaves a workgroup without a stage; the whole-workgroup shape has as many full stages in
    every workgroup"""
    for n in NS:
        for m in ms_of(n):
            p = keep_plan(m, n)
            assert (p["family"], p["flat"]) == (("fdp", 1) if n == 100 else ("fdp_nw", 0)), (m, n, p)
        m = m_with_idle_workgroups(n)
        assert m % 2 == 0 and grid(m, n) > 1 and stages_of_last_workgroup(m, n) == 0, (n, m)
        m = m_of_whole_workgroups(n)
        assert m % (RS * grid(m, n)) == 0 and grid(m, n) >= 2, (n, m)


@pytest.mark.parametrize("n,off", [(33, 0), (127, 0), (64, 1), (128, 1)])
def test_flat_producer_paths_keep_agreeing(n, off):
    """odd n and an offset view: the flat producer (the parent's code) with J = NULL against its J-buffer run"""
    for m in (1, 65, 1031):
        p = keep_plan(m, n, off == 0)
        assert (p["family"], p["flat"]) == ("fdp", 1), (m, n, off, p)
        for collapsed in (False, True):
            check_shape(m, n, collapsed, off)
