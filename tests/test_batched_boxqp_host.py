"""Batched box-constrained QP solves (mir_lsq_batched_box_qp_s / _d, M.solveBoxQPBatched), CPU tier: the entries are exported
and declared, their argument checks answer without a device, the Python wrapper validates and pads to the 8-wide layout
without one, and the case families of tests/boxqp_cases.py keep what the device tests rely on -- conditioning, the cap on
margin-screened-out problems, mixed waves of 0 / 1 / 2 / >= 3 iterations, the KKT tolerance on the oracle's own solutions --
by the oracle alone."""
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


def test_entries_are_exported_declared_and_built_as_a_unit_of_their_own():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    for name in ("mir_lsq_batched_box_qp_s", "mir_lsq_batched_box_qp_d"):
        assert getattr(L, name)
        assert re.search(r"\bint\s+" + name + r"\(", header), name
    assert re.search(r"#define\s+MIR_LSQ_BOX_QP_UNCONSTRAINED_SOLUTION\s+1u", header)
    assert api.BOX_QP_UNCONSTRAINED_SOLUTION == 1
    from mir_optim_amd import build as hipbuild
    assert "launch_boxqp.hip" in hipbuild.SOLVER_UNITS
    assert callable(M.solveBoxQPBatched)


@pytest.mark.parametrize("suffix, dtype", PRECISIONS)
def test_argument_checks_need_no_device(suffix, dtype):
    fn = getattr(api.lib(), "mir_lsq_batched_box_qp" + suffix)
    s = M.BoxQPSettings(dtype)
    P = np.zeros((2, 8, 8), dtype); q = np.zeros((2, 8), dtype); l = np.zeros(8, dtype); u = np.zeros(8, dtype)
    x = np.zeros((2, 8), dtype); st = np.zeros(2, np.int32); it = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data
    good = [C.addressof(s), 2, 3, p(P), p(q), p(l), p(u), 0, p(x), p(st), p(it), 0, None]
    for k in (0, 3, 4, 5, 6, 8, 9):                            # every required pointer, one at a time
        bad = list(good); bad[k] = None
        assert fn(*bad) == -1, k
    for n in (0, 9, 16):
        bad = list(good); bad[2] = n
        assert fn(*bad) == -1, n
    for stride in (1, 3, 7, 16):                               # bound_stride is 0 or 8
        bad = list(good); bad[7] = stride
        assert fn(*bad) == -1, stride
    nothing = list(good); nothing[1] = 0                       # count == 0: nothing to do, nothing launched
    assert fn(*nothing) == 0
    nothing[10] = None                                         # iterations may be NULL
    assert fn(*nothing) == 0


def test_wrapper_validates_and_pads_without_a_device():
    rng = np.random.default_rng(5)
    P = rng.standard_normal((3, 5, 5)); q = rng.standard_normal((3, 5))
    l = -np.ones(5); u = np.ones((3, 5))
    count, n, Pp, qp, lp, up, stride, xp = api._box_qp_batched_pack(P, q, l, np.ones(5), None, np.float64, False)
    assert (count, n, stride) == (3, 5, 0) and Pp.shape == (3, 8, 8) and qp.shape == xp.shape == (3, 8) and lp.shape == up.shape == (8,)
    assert np.array_equal(Pp[:, :5, :5], P) and not Pp[:, 5:, :].any() and not Pp[:, :, 5:].any()
    assert np.array_equal(qp[:, :5], q) and not qp[:, 5:].any() and np.array_equal(lp[:5], l) and not xp.any()
    count, n, Pp, qp, lp, up, stride, xp = api._box_qp_batched_pack(P, q, -u, u, q, np.float32, True)
    assert stride == 8 and lp.shape == up.shape == (3, 8) and Pp.dtype == np.float32 and np.array_equal(xp[:, :5], q.astype(np.float32))
    with pytest.raises(ValueError):
        api._box_qp_batched_pack(P[0], q, l, l, None, np.float64, False)              # P is count x n x n
    with pytest.raises(ValueError):
        api._box_qp_batched_pack(np.zeros((2, 9, 9)), np.zeros((2, 9)), np.zeros(9), np.zeros(9), None, np.float64, False)
    with pytest.raises(ValueError):
        api._box_qp_batched_pack(P, q[:2], l, l, None, np.float64, False)
    with pytest.raises(ValueError):
        api._box_qp_batched_pack(P, q, l, u, None, np.float64, False)                 # l shared, u per problem
    with pytest.raises(ValueError):
        api._box_qp_batched_pack(P, q, l[:4], l[:4], None, np.float64, False)
    with pytest.raises(ValueError):
        api._box_qp_batched_pack(P, q, l, l, None, np.float64, True)                  # the flag needs x
    with pytest.raises(ValueError):
        api._box_qp_batched_pack(P, q, l, l, None, np.int32, False)
    st, x, it = M.solveBoxQPBatched(np.zeros((0, 4, 4)), np.zeros((0, 4)), np.zeros(4), np.ones(4))     # no device touched
    assert st.shape == (0,) and x.shape == (0, 4) and it.shape == (0,)


@pytest.mark.parametrize("n", B.NS)
def test_families_are_seeded_and_well_conditioned(n):
    for dtype in B.DTYPES:
        P, q, l, u = B.family(n, dtype)
        assert P.shape == (B.FAMILY_COUNT, n, n) and q.shape == l.shape == u.shape == (B.FAMILY_COUNT, n)
        assert all(B.cond2(Pp) <= 1e3 for Pp in P) and np.array_equal(P, np.swapaxes(P, 1, 2)) and np.all(l < u)
        assert np.array_equal(P.astype(dtype).astype(np.float64), P)                  # representable in dtype
        B.family.cache_clear()
        assert all(np.array_equal(a, b) for a, b in zip(B.family(n, dtype), (P, q, l, u)))


@pytest.mark.parametrize("n", B.NS)
@pytest.mark.parametrize("dtype", B.DTYPES, ids=["f32", "f64"])
def test_the_oracle_alone_keeps_the_screened_out_share_within_the_cap(oracle, n, dtype):
    """The margin screen (boxqp_cases) may take at most 10 % of a family out of the exact status / iteration / active-set
    comparison; the rest must really exercise the loop: solved, most with an active bound, and the float oracle must take the
    f64 oracle's path on every screened problem (else the screen would not separate rounding from a wrong loop)."""
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


@pytest.mark.parametrize("n", B.NS)
@pytest.mark.parametrize("dtype", B.DTYPES, ids=["f32", "f64"])
def test_the_kkt_tolerance_holds_for_the_oracles_own_solutions(oracle, n, dtype):
    """tau_i = 8 eps(T) (|P||x| + |q|)_i is the device test's KKT tolerance; the same-precision oracle's x must pass it with room
    (the rule: if the oracle needed more than 8, the factor would be twice the oracle's need)."""
    P, q, l, u = B.family(n, dtype)
    st, x, it = B.oracle_family(oracle, n, dtype)
    need = max(B.kkt_factor(P[p], q[p], l[p], u[p], x[p], np.finfo(dtype).eps) for p in range(B.FAMILY_COUNT))
    print(f"n = {n} {np.dtype(dtype).name}: the oracle needs a factor of {need:.2f}")
    assert need <= B.KKT_FACTOR


@pytest.mark.parametrize("n", B.NS)
@pytest.mark.parametrize("dtype", B.DTYPES, ids=["f32", "f64"])
def test_the_mixed_wave_search_finds_its_classes(oracle, n, dtype):
    found = B.mixed_wave(oracle, n, dtype)
    assert sorted(found) == ([0, 1] if n == 1 else [0, 1, 2, 3])
    for cls, (P, q, l, u) in found.items():
        st, x, it = oracle.solve_box_qp(np.tril(P), q, l, u, dtype=dtype)
        assert st == 0 and min(it, 3) == cls and B.cond2(P) <= 1e3
