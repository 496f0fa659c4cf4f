"""Batched box-constrained QP solves of order 9 .. 16 (mir_lsq_batched_box_qp16_s / _d, M.solveBoxQPBatched at n > 8), CPU
tier: the four entries are exported and declared, their argument checks answer without a device, the Python wrapper validates
and pads to the 16-wide layout without one, and the case families of tests/boxqp_cases.py keep at n = 9, 13, 16 what the
device tests (tests/test_gpu_batched_boxqp16.py) rely on -- conditioning, the cap on margin-screened-out problems, mixed waves,
the KKT tolerance on the oracle's own solutions -- by the oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api
import boxqp_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [pytest.param("_s", np.float32, id="f32"), pytest.param("_d", np.float64, id="f64")]
NS16 = B.NS16
DTYPES = pytest.mark.parametrize("dtype", B.DTYPES, ids=["f32", "f64"])


def test_entries_are_exported_declared_and_built_as_units_of_their_own():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    for name in ("mir_lsq_batched_box_qp16_s", "mir_lsq_batched_box_qp16_d", "mir_lsq_batched_posvx16_s", "mir_lsq_batched_posvx16_d"):
        assert getattr(L, name)
        assert re.search(r"\bint\s+" + name + r"\(", header), name
    from mir_optim_amd import build as hipbuild
    assert "launch_boxqp16_s.hip" in hipbuild.SOLVER_UNITS and "launch_boxqp16_d.hip" in hipbuild.SOLVER_UNITS
    assert "launch_boxqp.hip" in hipbuild.SOLVER_UNITS


@pytest.mark.parametrize("suffix, dtype", PRECISIONS)
def test_argument_checks_need_no_device(suffix, dtype):
    fn = getattr(api.lib(), "mir_lsq_batched_box_qp16" + suffix)
    s = M.BoxQPSettings(dtype)
    P = np.zeros((2, 16, 16), dtype); q = np.zeros((2, 16), dtype); l = np.zeros(16, dtype); u = np.zeros(16, dtype)
    x = np.zeros((2, 16), dtype); st = np.zeros(2, np.int32); it = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data
    good = [C.addressof(s), 2, 12, p(P), p(q), p(l), p(u), 0, p(x), p(st), p(it), 0, None]
    for k in (0, 3, 4, 5, 6, 8, 9):                            # every required pointer, one at a time
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    for n in (0, 8, 17):
        bad = list(good); bad[2] = n
        assert fn(*bad) == -1, n
    for stride in (1, 8, 15, 17):                              # bound_stride is 0 or 16
        bad = list(good); bad[7] = stride
        assert fn(*bad) == -1, stride
    nothing = list(good); nothing[1] = 0                       # count == 0: nothing to do, nothing launched
    assert fn(*nothing) == 0
    nothing[10] = None                                         # iterations may be NULL
    assert fn(*nothing) == 0


def test_wrapper_validates_and_pads_without_a_device():
    rng = np.random.default_rng(5)
    P = rng.standard_normal((3, 13, 13)); q = rng.standard_normal((3, 13))
    l = -np.ones(13); u = np.ones((3, 13))
    count, n, Pp, qp, lp, up, stride, xp = api._box_qp_batched_pack16(P, q, l, np.ones(13), None, np.float64, False)
    assert (count, n, stride) == (3, 13, 0) and Pp.shape == (3, 16, 16) and qp.shape == xp.shape == (3, 16)
    assert lp.shape == up.shape == (16,) and Pp.dtype == np.float64
    assert np.array_equal(Pp[:, :13, :13], P) and not Pp[:, 13:, :].any() and not Pp[:, :, 13:].any()
    assert np.array_equal(qp[:, :13], q) and not qp[:, 13:].any() and np.array_equal(lp[:13], l) and not lp[13:].any()
    assert np.array_equal(up[:13], np.ones(13)) and not up[13:].any() and not xp.any()
    count, n, Pp, qp, lp, up, stride, xp = api._box_qp_batched_pack16(P, q, -u, u, q, np.float32, True)
    assert stride == 16 and lp.shape == up.shape == (3, 16) and Pp.dtype == qp.dtype == lp.dtype == xp.dtype == np.float32
    assert np.array_equal(xp[:, :13], q.astype(np.float32)) and not xp[:, 13:].any()
    assert np.array_equal(up[:, :13], u.astype(np.float32)) and not up[:, 13:].any() and not lp[:, 13:].any()
    with pytest.raises(ValueError):
        api._box_qp_batched_pack16(P[0], q, l, l, None, np.float64, False)            # P is count x n x n
    with pytest.raises(ValueError, match="16"):
        api._box_qp_batched_pack16(np.zeros((2, 17, 17)), np.zeros((2, 17)), np.zeros(17), np.zeros(17), None, np.float64, False)
    with pytest.raises(ValueError):
        api._box_qp_batched_pack16(P, q[:2], l, l, None, np.float64, False)
    with pytest.raises(ValueError):
        api._box_qp_batched_pack16(P, q, l, u, None, np.float64, False)               # l shared, u per problem
    with pytest.raises(ValueError):
        api._box_qp_batched_pack16(P, q, l[:4], l[:4], None, np.float64, False)
    with pytest.raises(ValueError):
        api._box_qp_batched_pack16(P, q, l, l, None, np.float64, True)                # the flag needs x
    with pytest.raises(ValueError):
        api._box_qp_batched_pack16(P, q, l, l, None, np.int32, False)
    with pytest.raises(ValueError, match="16"):                                       # the wrapper names the limit
        M.solveBoxQPBatched(np.zeros((2, 17, 17)), np.zeros((2, 17)), np.zeros(17), np.ones(17))
    for dtype in B.DTYPES:                                                            # no device touched
        st, x, it = M.solveBoxQPBatched(np.zeros((0, 12, 12)), np.zeros((0, 12)), np.zeros(12), np.ones(12), dtype=dtype)
        assert st.shape == (0,) and x.shape == (0, 12) and it.shape == (0,) and x.dtype == dtype


@pytest.mark.parametrize("n", NS16)
def test_families_are_seeded_and_well_conditioned(n):
    for dtype in B.DTYPES:
        P, q, l, u = B.family(n, dtype)
        assert P.shape == (B.FAMILY_COUNT, n, n) and q.shape == l.shape == u.shape == (B.FAMILY_COUNT, n)
        assert all(B.cond2(Pp) <= 1e3 for Pp in P) and np.array_equal(P, np.swapaxes(P, 1, 2)) and np.all(l < u)
        assert np.array_equal(P.astype(dtype).astype(np.float64), P)                  # representable in dtype


@pytest.mark.parametrize("n", NS16)
@DTYPES
def test_the_oracle_alone_keeps_the_screened_out_share_within_the_cap(oracle, n, dtype):
    """As tests/test_batched_boxqp_host.py asks of the n <= 8 families: at most 10 % of a family fails the margin screen, every
    problem is solved by both oracles, most take active-set steps, and the float oracle takes the f64 oracle's path on every
    screened problem."""
    P, q, l, u = B.family(n, dtype)
    keep = B.screen_family(oracle, n, dtype)
    out = B.FAMILY_COUNT - int(keep.sum())
    print(f"n = {n} {np.dtype(dtype).name}: {out} of {B.FAMILY_COUNT} screened out")
    assert out <= B.MAX_SCREENED_OUT * B.FAMILY_COUNT
    st, x, it = B.oracle_family(oracle, n, dtype)
    st64, x64, it64 = B.oracle_family(oracle, n, np.float64, dtype)
    assert np.all(st == 0) and np.all(st64 == 0)
    assert np.mean(it > 0) >= 0.5
    assert np.array_equal(it[keep], it64[keep]) and np.array_equal(B.active_set(x, l, u)[keep], B.active_set(x64, l, u)[keep])


@pytest.mark.parametrize("n", NS16)
@DTYPES
def test_the_kkt_tolerance_holds_for_the_oracles_own_solutions(oracle, n, dtype):
    P, q, l, u = B.family(n, dtype)
    st, x, it = B.oracle_family(oracle, n, dtype)
    need = max(B.kkt_factor(P[p], q[p], l[p], u[p], x[p], np.finfo(dtype).eps) for p in range(B.FAMILY_COUNT))
    print(f"n = {n} {np.dtype(dtype).name}: the oracle needs a factor of {need:.2f}")
    assert need <= B.KKT_FACTOR


def class0_at_16(found):
    """the class-0 member of the n = 16 mixed wave: the class-1 problem with bounds +-1e3 (its unconstrained minimiser is
    feasible then); the device test builds the same"""
    P, q, l, u = found[1]
    return P, q, np.full(16, -1e3), np.full(16, 1e3)


@pytest.mark.parametrize("n", NS16)
@DTYPES
def test_the_mixed_wave_search_finds_its_classes(oracle, n, dtype):
    """n = 9, 13: the classes 0, 1, 2, >= 3 with the default budget. n = 16: a feasible unconstrained minimiser is too rare for
    the search, which finds 1, 2, >= 3; class 0 is the class-1 problem with bounds +-1e3: solved, 0 iterations, margin screened."""
    found = B.mixed_wave(oracle, n, dtype)
    assert sorted(found) == ([1, 2, 3] if n == 16 else [0, 1, 2, 3])
    for cls, (P, q, l, u) in found.items():
        st, x, it = oracle.solve_box_qp(np.tril(P), q, l, u, dtype=dtype)
        assert st == 0 and min(it, 3) == cls and B.cond2(P) <= 1e3
    if n == 16:
        P, q, l, u = class0_at_16(found)
        st, x, it = oracle.solve_box_qp(np.tril(P), q, l, u, dtype=dtype)
        st64, x64, it64 = oracle.solve_box_qp(np.tril(P), q, l, u)
        assert (st, it) == (0, 0) and (st64, it64) == (0, 0) and B.margin_screened(P, q, l, u, x64)
