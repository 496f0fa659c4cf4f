"""Batched box-constrained QP solves of order 17 .. 64 (mir_lsq_batched_box_qp64_s / _d, M.solveBoxQPBatchedWide), CPU tier:
the four entries are exported and declared and their units are built, the argument checks answer without a device, a call
without a device returns -5, the Python wrapper validates and packs the dense layout without one, and the case families of
tests/boxqp_cases.py keep at n = 17, 31, 32, 33, 63, 64 what the device tests (tests/test_gpu_batched_boxqp64.py) rely on, by
the oracle alone: at most 2 of 64 problems fail the margin screen at SINGLE_MARGIN (float 3e-5, double 1e-8), the float oracle
takes the f64 oracle's path on the rest, the mixed-wave search finds its classes, every-bound-active and indefinite problems do
what their constructions say."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api
import boxqp_cases as B
import boxqp64_cases as B64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [pytest.param("_s", np.float32, id="f32"), pytest.param("_d", np.float64, id="f64")]
DTYPES = pytest.mark.parametrize("dtype", B.DTYPES, ids=["f32", "f64"])
ENTRIES = ("mir_lsq_batched_box_qp64_s", "mir_lsq_batched_box_qp64_d", "mir_lsq_batched_box_qp64_waves_s",
           "mir_lsq_batched_box_qp64_waves_d")


def test_entries_are_exported_declared_and_built_as_units_of_their_own():
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "mir_optim_amd.h")).read()
    for name in ENTRIES:
        assert getattr(L, name)
        assert re.search(r"\bint\s+" + name + r"\(", header), name
    from mir_optim_amd import build as hipbuild
    assert "launch_boxqp64_s.hip" in hipbuild.SOLVER_UNITS and "launch_boxqp64_d.hip" in hipbuild.SOLVER_UNITS
    for unit in ("launch_boxqp.hip", "launch_boxqp16_s.hip", "launch_boxqp16_d.hip"):
        assert unit in hipbuild.SOLVER_UNITS
    assert L.mir_lsq_version().decode().startswith("mir_optim_amd 0.4")                  # callers discover the symbols by name
    assert "solveBoxQPBatchedWide" in api.__all__ and M.solveBoxQPBatchedWide is api.solveBoxQPBatchedWide


def good_arguments(dtype, n=40):
    s = M.BoxQPSettings(dtype)
    keep = [s, np.zeros((2, n, n), dtype), np.zeros((2, n), dtype), np.zeros(n, dtype), np.zeros(n, dtype), np.zeros((2, n), dtype),
            np.zeros(2, np.int32), np.zeros(2, np.int32)]
    p = lambda a: a.ctypes.data
    P, q, l, u, x, st, it = keep[1:]
    return keep, [C.addressof(s), 2, n, p(P), p(q), p(l), p(u), 0, p(x), p(st), p(it), 0, None]


@pytest.mark.parametrize("waves", [False, True], ids=["public", "waves"])
@pytest.mark.parametrize("suffix, dtype", PRECISIONS)
def test_argument_checks_need_no_device(suffix, dtype, waves):
    fn = getattr(api.lib(), ("mir_lsq_batched_box_qp64_waves" if waves else "mir_lsq_batched_box_qp64") + suffix)
    keep, good = good_arguments(dtype)
    tail = [0] if waves else []
    for k in (0, 3, 4, 5, 6, 8, 9):                            # every required pointer, one at a time
        bad = list(good); bad[k] = None
        assert fn(*bad, *tail) == -1, k
    for n in (0, 1, 8, 16, 65, 128):
        bad = list(good); bad[2] = n
        assert fn(*bad, *tail) == -1, n
    for stride in (1, 16, 39, 41, 64):                         # bound_stride is 0 or n
        bad = list(good); bad[7] = stride
        assert fn(*bad, *tail) == -1, stride
    bad = list(good); bad[1] = (1 << 30) + 1
    assert fn(*bad, *tail) == -1
    for n in (17, 32, 33, 64):                                 # count == 0: nothing to do, nothing launched, no device needed
        nothing = list(good); nothing[1] = 0; nothing[2] = n
        assert fn(*nothing, *tail) == 0
        nothing[7] = n
        assert fn(*nothing, *tail) == 0
        nothing[10] = None                                     # iterations may be NULL
        assert fn(*nothing, *tail) == 0


NO_DEVICE = """
import ctypes as C, sys
import numpy as np
sys.path.insert(0, {root!r})
import mir_optim_amd as M
from mir_optim_amd import api
assert M.device_count() == 0
for suffix, dtype in (("_s", np.float32), ("_d", np.float64)):
    for n in (17, 64):
        s = M.BoxQPSettings(dtype)
        P = np.zeros((2, n, n), dtype); q = np.zeros((2, n), dtype); l = np.zeros(n, dtype); u = np.zeros(n, dtype)
        x = np.zeros((2, n), dtype); st = np.zeros(2, np.int32); it = np.zeros(2, np.int32)
        p = lambda a: a.ctypes.data
        args = [C.addressof(s), 2, n, p(P), p(q), p(l), p(u), 0, p(x), p(st), p(it), 0, None]
        assert getattr(api.lib(), "mir_lsq_batched_box_qp64" + suffix)(*args) == -5
        assert getattr(api.lib(), "mir_lsq_batched_box_qp64_waves" + suffix)(*args, 1) == -5
print("no device: -5")
"""


def test_without_a_device_the_call_returns_minus_5():
    """in a child process that sees no device, whatever this machine has"""
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", NO_DEVICE.format(root=ROOT)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and "no device: -5" in p.stdout.decode(), p.stderr.decode()[-2000:]


def test_wrapper_validates_and_packs_without_a_device():
    rng = np.random.default_rng(5)
    n = 21
    P = rng.standard_normal((3, n, n)); q = rng.standard_normal((3, n))
    l = -np.ones(n); u = np.ones((3, n))
    pack = api._box_qp_batched_pack_dense
    count, n_, Pp, qp, lp, up, stride, xp = pack(P, q, l, np.ones(n), None, np.float64, False)
    assert (count, n_, stride) == (3, n, 0) and Pp.shape == (3, n, n) and qp.shape == xp.shape == (3, n)
    assert lp.shape == up.shape == (n,) and Pp.dtype == qp.dtype == lp.dtype == up.dtype == xp.dtype == np.float64
    assert np.array_equal(Pp, P) and np.array_equal(qp, q) and np.array_equal(lp, l) and np.array_equal(up, np.ones(n)) and not xp.any()
    assert all(a.flags.c_contiguous for a in (Pp, qp, lp, up, xp))
    Pt = np.swapaxes(P, 1, 2)                                                          # not contiguous: the pack copies
    count, n_, Pp, qp, lp, up, stride, xp = pack(Pt, q, -u, u, q, np.float32, True)
    assert stride == n and lp.shape == up.shape == (3, n) and Pp.dtype == qp.dtype == lp.dtype == up.dtype == xp.dtype == np.float32
    assert Pp.flags.c_contiguous and np.array_equal(Pp, Pt.astype(np.float32)) and np.array_equal(xp, q.astype(np.float32))
    assert np.array_equal(up, u.astype(np.float32)) and np.array_equal(lp, -u.astype(np.float32))
    xp[0, 0] = 7.0
    assert q[0, 0] != 7.0                                                              # x is a copy: the caller's array stays
    with pytest.raises(ValueError):
        pack(P[0], q, l, l, None, np.float64, False)                                   # P is count x n x n
    for bad in (16, 65):
        with pytest.raises(ValueError, match="17 .. 64"):
            pack(np.zeros((2, bad, bad)), np.zeros((2, bad)), np.zeros(bad), np.zeros(bad), None, np.float64, False)
        with pytest.raises(ValueError, match="17 .. 64"):                              # the wrapper names the range
            M.solveBoxQPBatchedWide(np.zeros((2, bad, bad)), np.zeros((2, bad)), np.zeros(bad), np.ones(bad))
    with pytest.raises(ValueError):
        pack(P, q[:2], l, l, None, np.float64, False)
    with pytest.raises(ValueError):
        pack(P, q, l, u, None, np.float64, False)                                      # l shared, u per problem
    with pytest.raises(ValueError):
        pack(P, q, l[:4], l[:4], None, np.float64, False)
    with pytest.raises(ValueError):
        pack(P, q, l, l, q[:2], np.float64, True)                                      # x is count x n
    with pytest.raises(ValueError):
        pack(P, q, l, l, None, np.float64, True)                                       # the flag needs x
    with pytest.raises(ValueError):
        pack(P, q, l, l, None, np.int32, False)
    for dtype in B.DTYPES:                                                             # no device touched
        st, x, it = M.solveBoxQPBatchedWide(np.zeros((0, 40, 40)), np.zeros((0, 40)), np.zeros(40), np.ones(40), dtype=dtype)
        assert st.shape == (0,) and x.shape == (0, 40) and it.shape == (0,) and x.dtype == dtype
    with pytest.raises(ValueError, match="16"):                                        # the old name keeps its limit
        M.solveBoxQPBatched(np.zeros((2, 17, 17)), np.zeros((2, 17)), np.zeros(17), np.ones(17))


@pytest.mark.parametrize("n", B64.NS64)
@DTYPES
def test_the_oracle_alone_keeps_the_screened_out_problems_within_the_cap(oracle, n, dtype):
    """At SINGLE_MARGIN at most 2 of 64 problems fail the screen; both oracles solve every problem, every problem takes
    active-set steps, and the float oracle takes the f64 oracle's status, iterations and active set on every screened problem."""
    P, q, l, u = B64.fam(n, dtype)
    assert P.shape == (B64.COUNT, n, n) and all(B.cond2(Pp) <= 1e3 for Pp in P)
    keep = B64.screen(oracle, n, dtype)
    out = B64.COUNT - int(keep.sum())
    (st, x, it), (st64, x64, it64) = B64.oracles(oracle, n, dtype)
    print(f"n = {n} {np.dtype(dtype).name}: {out} of {B64.COUNT} screened out, iterations {it.min()} .. {it.max()}, "
          f"{np.mean(B.active_set(x64, l, u) != 0):.2f} of the variables on a bound, largest distance {np.abs(x - x64).max():.2e}")
    assert out <= B64.MAX_SCREENED_OUT
    assert np.all(st == 0) and np.all(st64 == 0) and np.all(it > 0)
    assert np.array_equal(it[keep], it64[keep]) and np.array_equal(B.active_set(x, l, u)[keep], B.active_set(x64, l, u)[keep])
    need = max(B.kkt_factor(P[p], q[p], l[p], u[p], x[p], np.finfo(dtype).eps) for p in range(B64.COUNT))
    assert need <= B.KKT_FACTOR


@pytest.mark.parametrize("n", B64.NS_W32)
@DTYPES
def test_the_mixed_wave_search_finds_its_classes(oracle, n, dtype):
    """A feasible unconstrained minimiser is too rare at these orders for the search, which finds 1, 2, >= 3 iterations; class
    0 is the class-1 problem with bounds +-1e3: solved, 0 iterations, margin screened."""
    found = B.mixed_wave(oracle, n, dtype)
    assert sorted(found) == [1, 2, 3]
    for cls, (P, q, l, u) in found.items():
        st, x, it = oracle.solve_box_qp(np.tril(P), q, l, u, dtype=dtype)
        assert st == 0 and min(it, 3) == cls and B.cond2(P) <= 1e3
    P, q, l, u = B64.class0(found, n)
    st, x, it = oracle.solve_box_qp(np.tril(P), q, l, u, dtype=dtype)
    st64, x64, it64 = oracle.solve_box_qp(np.tril(P), q, l, u)
    assert (st, it) == (0, 0) and (st64, it64) == (0, 0) and B.margin_screened(P, q, l, u, x64)


@pytest.mark.parametrize("n", B64.NS64)
@DTYPES
def test_every_bound_active_and_indefinite_constructions(oracle, n, dtype):
    P, q, l, u, _ = B.all_active_family(n, dtype)
    so, xo, io = B.oracle_solve(oracle, P, q, l, u, dtype)
    assert np.all(so == 0) and np.all(io == 1) and np.array_equal(xo, l)
    P, q, l, u = (a[:4] for a in B64.fam(n, dtype))
    for k in B.indefinite_positions(n):
        for p in range(len(q)):
            so = oracle.solve_box_qp(np.tril(B.indefinite(P[p], k)), q[p], l[p], u[p], dtype=dtype)[0]
            assert so == M.BoxQPStatus.numericError, (k, p)


@pytest.mark.parametrize("n", B64.NS64)
def test_equal_bounds_oracles_agree_under_the_iteration_limit(oracle, n):
    """l == u in every component and in the even ones, maxIterations = 64: the float and the f64 oracle agree in status and
    iteration count on the float families, which is what lets the device test compare both exactly."""
    P, q, l, u = B64.fam(n, np.float32)
    c = B.equal_bounds_centre(l, u, np.float32)
    for fixed in (np.ones(n, bool), np.arange(n) % 2 == 0):
        lf, uf = np.where(fixed, c, l), np.where(fixed, c, u)
        res = [B.oracle_solve(oracle, P, q, lf, uf, dt, settings=B.qp_settings(oracle, dt, maxIterations=B.EQUAL_BOUNDS_MAX_ITERATIONS))
               for dt in (np.float32, np.float64)]
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][2], res[1][2])
