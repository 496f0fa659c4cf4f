"""The one-problem BOXCQP entry on the device (M.solveBoxQP -> mir_solve_box_qp_gpu_s / _d -> box_qp_device of
csrc/solve_kernel.h, the box QP of every bounded pass of the general LM solver too) against oracle.solve_box_qp, in both
precisions, at the orders where its kernels change shape: k_box_qp<T, NB> with the factor in LDS (NB = 1, 2, 4, 8: n <= 16 /
32 / 64 / 128; solve_lds.h), NB = 0 with potrf_panel and the factor in global memory (129 .. 256), k_box_qp_big above
(solve_big.h). boxqp_cases.NS_SINGLE has both sides of every class edge, one short of a full 16-row block, and 1, 2, 300;
EDGE_NS both sides of every edge. 16 problems an order (boxqp_cases.family), each call one launch, P handed in as its lower
triangle with NaN above (QP:109).

The discipline is that of the batched kernels' tests (tests/test_gpu_batched_boxqp.py), through the same
boxqp_cases.check_against_oracle:
  * status equals the same-precision oracle's; on margin-screened problems so do the iteration count and the active set. The
    screen is boxqp_cases.SINGLE_MARGIN (float 3e-5, double 1e-8; why not 1e-3: boxqp_cases), and
    tests/test_boxqp_single_host.py keeps on the CPU that it drops at most 2 of 16 problems and that the float oracle takes the
    f64 oracle's path on the rest;
  * an independent KKT check of the device's x in numpy float64 with the factor 8 (the oracle's own x: at most 1.37);
  * distance to the f64 oracle on the same (rounded) data: double 8 eps cond_2(P) max|x|, of which the f64 oracle itself uses
    under 1 % from n = 15 on (CPU tier); float 4 x the float oracle's own largest distance, floor 4 eps max|x|.
Beyond the family: a second call gives the same bits (scratch is allocated afresh each call, so a read of uninitialised scratch
or LDS would show), non-default classification tolerances, unconstrainedSolution = true, infinite bounds against a box of
+-1e3, float ?posvx on badly scaled rows, every bound active (s == 0, no reduced solve), l == u, an indefinite P with the bad
pivot in the first block, at a block edge, in the middle and at the end, and nothing lingering after it, maxIterations = 1 and
a NaN in q (quirk Q8).

Measured on an MI355X with this file (worst over the orders of a class, 16 problems each; KKT factor needed / largest distance
over its tolerance):
  class (orders run)              float32          float64
  k_box_qp<NB=1> (1, 2, 15, 16)   0.49 / 0.289     0.83 / 0.121 (n = 1; 0.008 at n = 15, 16)
  k_box_qp<NB=2> (17, 31, 32)     0.88 / 0.462     0.82 / 0.004
  k_box_qp<NB=4> (33, 63, 64)     0.51 / 0.256     0.92 / 0.007
  k_box_qp<NB=8> (65, 127, 128)   0.53 / 0.208     0.96 / 0.006
  k_box_qp<NB=0> (129, 255, 256)  0.76 / 0.261     1.25 / 0.006
  k_box_qp_big (257, 300)         0.96 / 0.316     1.52 / 0.010
Badly scaled float rows (test_float_posvx_on_badly_scaled_rows): the device's largest relative error 2.3e-7 .. 2.5e-6 over
EDGE_NS, the float oracle's 1.7e-7 .. 1.8e-6; the device's largest over the oracle's largest at most 1.6 (n = 128).
"""
import numpy as np
import pytest

import mir_optim_amd as M
import boxqp_cases as B
from boxqp_cases import check_against_oracle, same_bits, solve_single, x_tolerance

pytestmark = pytest.mark.gpu

DT = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
COUNT = B.SINGLE_COUNT
_DEVICE = {}


def fam(n, dtype):
    return B.family(n, dtype, count=COUNT)


def device_family(n, dtype):
    """the device's answers on the family with default settings, computed once and shared (read-only)"""
    key = (n, np.dtype(dtype).name)
    if key not in _DEVICE:
        res = solve_single(*fam(n, dtype), dtype)
        for a in res:
            a.setflags(write=False)
        _DEVICE[key] = res
    return _DEVICE[key]


def oracles(oracle, n, dtype):
    return B.oracle_family(oracle, n, dtype, count=COUNT), B.oracle_family(oracle, n, np.float64, dtype, COUNT)


def screen(oracle, n, dtype):
    return B.screen_family(oracle, n, dtype, B.SINGLE_MARGIN[dtype], COUNT)


# ---------------------------------------------------------------- 1, 2: the family, and the same bits from a second call
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS_SINGLE)
def test_family_matches_the_oracle(oracle, n, dtype):
    data = fam(n, dtype)
    dev = device_family(n, dtype)
    ora, ora64 = oracles(oracle, n, dtype)
    kkt, ratio = B.worst_figures(dev, ora, ora64, data, dtype)
    print(f"{B.kernel_class(n)} {np.dtype(dtype).name} n = {n}: KKT factor {kkt:.2f}, distance / tolerance {ratio:.4f}, "
          f"iterations {dev[2].min()} .. {dev[2].max()}")
    check_against_oracle(dev, ora, ora64, data, dtype, screen(oracle, n, dtype))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS_SINGLE)
def test_a_second_call_gives_the_same_bits(n, dtype):
    first = device_family(n, dtype)
    again = solve_single(*fam(n, dtype), dtype)
    assert same_bits(again, first)


# ---------------------------------------------------------------- 3, 4: settings and the handed-in unconstrained solution
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.EDGE_NS)
@pytest.mark.parametrize("rel", ["16eps", 1e-6])
@pytest.mark.parametrize("ab", ["16eps", 1e-6])
def test_non_default_classification_tolerances(oracle, n, dtype, rel, ab):
    eps = float(np.finfo(dtype).eps)
    rel, ab = (16 * eps if v == "16eps" else v for v in (rel, ab))
    data = fam(n, dtype)
    s = M.BoxQPSettings(dtype); s.relTolerance = rel; s.absTolerance = ab
    dev = solve_single(*data, dtype, settings=s)
    ora = B.oracle_solve(oracle, *data, dtype, settings=B.qp_settings(oracle, dtype, relTolerance=rel, absTolerance=ab))
    ora64 = B.oracle_solve(oracle, *data, np.float64, settings=B.qp_settings(oracle, np.float64, relTolerance=rel, absTolerance=ab))
    check_against_oracle(dev, ora, ora64, data, dtype, screen(oracle, n, dtype))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.EDGE_NS)
def test_handing_in_the_unconstrained_solution(oracle, n, dtype):
    """unconstrainedSolution = true with x = the same-precision oracle's unconstrained solution: status and, on screened problems,
    iterations and active set as without the flag; and the oracle called the same way agrees."""
    data = fam(n, dtype)
    P, q, l, u = data
    inf = np.full(n, np.inf)
    s0, x0, _ = B.oracle_solve(oracle, P, q, -inf, inf, dtype)
    assert np.all(s0 == 0)
    plain = device_family(n, dtype)
    given = solve_single(*data, dtype, x=x0, unconstrainedSolution=True)
    scr = screen(oracle, n, dtype)
    assert np.array_equal(given[0], plain[0]) and np.array_equal(given[2][scr], plain[2][scr])
    assert np.array_equal(B.active_set(given[1], l, u)[scr], B.active_set(plain[1], l, u)[scr])
    ora = B.oracle_solve(oracle, *data, dtype, x0=x0)
    check_against_oracle(given, ora, B.oracle_family(oracle, n, np.float64, dtype, COUNT), data, dtype, scr)


# ---------------------------------------------------------------- 5, 6: no bound at all
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.EDGE_NS)
def test_infinite_bounds_and_a_huge_box(oracle, n, dtype):
    """status 0 and 0 iterations, x by the distance rule against oracle.posvx's solution (the KKT check with it), and the bits of
    the same problem inside a box of +-1e3 (the minimisers stay below 100: CPU tier)"""
    P, q, _, _ = fam(n, dtype)
    inf = np.full(n, np.inf)
    free = solve_single(P, q, -inf, inf, dtype)
    wide = solve_single(P, q, np.full(n, -1e3), np.full(n, 1e3), dtype)
    assert np.all(free[0] == 0) and np.all(free[2] == 0) and same_bits(free, wide)
    zero = np.zeros(COUNT, dtype=np.int32)
    sols = [[oracle.posvx(P[p], -q[p], dt) for p in range(COUNT)] for dt in (dtype, np.float64)]
    assert all(r["info"] == 0 for rs in sols for r in rs)
    ora, ora64 = ((zero, np.stack([r["x"] for r in rs]).astype(np.float64), zero) for rs in sols)
    L, U = np.tile(-inf, (COUNT, 1)), np.tile(inf, (COUNT, 1))
    check_against_oracle(free, ora, ora64, (P, q, L, U), dtype, np.ones(COUNT, bool))


@pytest.mark.parametrize("n", B.EDGE_NS)
def test_float_posvx_on_badly_scaled_rows(oracle, n):
    """D P D with D = 10^U(-1.5, 1.5) in float32 (equilibration must act), infinite bounds; the rule of
    test_unconstrained_solve_matches_oracle_posvx with eps32: against x*, the refined float64 solution of the rounded system, the
    device's error is at most 10 x the float oracle's + eps32, and the two differ by at most 4 max(err, err_oracle) + eps32
    (relative 2-norms)."""
    P, q = B.badly_scaled_family(n)
    inf = np.full(n, np.inf)
    eps = float(np.finfo(np.float32).eps)
    st, x, it = solve_single(P, q, -inf, inf, np.float32)
    so, xo, io = B.oracle_solve(oracle, P, q, -inf, inf, np.float32)
    assert np.all(st == 0) and np.all(so == 0) and np.all(it == 0) and np.all(io == 0)
    x = x.astype(np.float64)
    worst = [0.0, 0.0]
    for p in range(COUNT):
        xr = B.refined_solve(P[p], -q[p])
        err = np.linalg.norm(x[p] - xr) / np.linalg.norm(xr)
        erro = np.linalg.norm(xo[p] - xr) / np.linalg.norm(xr)
        worst = [max(worst[0], err), max(worst[1], erro)]
        assert err <= 10 * erro + eps, (p, err, erro)
        assert np.linalg.norm(x[p] - xo[p]) / np.linalg.norm(xo[p]) <= 4 * max(err, erro) + eps, (p, err, erro)
    print(f"{B.kernel_class(n)} n = {n}: largest relative error, device {worst[0]:.3e}, float oracle {worst[1]:.3e}")


# ---------------------------------------------------------------- 7, 8: every bound active, equal bounds
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.EDGE_NS)
def test_every_bound_active_takes_the_path_without_a_solve(oracle, n, dtype):
    P, q, l, u, _ = B.all_active_family(n, dtype)
    st, x, it = solve_single(P, q, l, u, dtype)
    so, xo, io = B.oracle_solve(oracle, P, q, l, u, dtype)
    assert np.all(so == 0) and np.all(io == 1) and np.array_equal(xo, l)           # the construction does what it says
    assert np.array_equal(st, so) and np.array_equal(it, io) and np.array_equal(x.astype(np.float64), l)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.EDGE_NS)
def test_equal_bounds(oracle, n, dtype):
    """l == u in every component (x is the bound, whatever the multipliers' signs), and in the even components only, with
    maxIterations = 64 on both sides: from n = 16 on the reference's loop cycles on most of these problems, on all of them from
    n = 64 on (boxqp_cases.EQUAL_BOUNDS_MAX_ITERATIONS; the CPU tier keeps that the limit changes no problem that ends). Then the
    status is maxIterations on both sides and x, the last iterate, still has its fixed components on the bound, as the oracle's."""
    P, q, l, u = fam(n, dtype)
    c = B.equal_bounds_centre(l, u, dtype)
    s = M.BoxQPSettings(dtype); s.maxIterations = B.EQUAL_BOUNDS_MAX_ITERATIONS
    so_ = lambda dt: B.qp_settings(oracle, dt, maxIterations=B.EQUAL_BOUNDS_MAX_ITERATIONS)
    for fixed in (np.ones(n, bool), np.arange(n) % 2 == 0):
        lf, uf = np.where(fixed, c, l), np.where(fixed, c, u)
        st, x, it = solve_single(P, q, lf, uf, dtype, settings=s)
        so, xo, io = B.oracle_solve(oracle, P, q, lf, uf, dtype, settings=so_(dtype))
        assert np.array_equal(st, so)
        ok = st == 0
        print(f"n = {n} {np.dtype(dtype).name}, {'every' if fixed.all() else 'even'} component fixed: {int(ok.sum())} of {COUNT} solved")
        assert np.array_equal(xo[:, fixed], c[:, fixed]) and np.array_equal(x.astype(np.float64)[:, fixed], c[:, fixed])
        if fixed.all():
            assert np.array_equal(it, io)
        else:
            s64, x64, _ = B.oracle_solve(oracle, P, q, lf, uf, np.float64, settings=so_(np.float64))
            both = ok & (s64 == 0)
            if both.any():                                     # the tolerance from the solved problems alone: a cycle's last
                tol = x_tolerance(dtype, P[both], x64[both], xo[both])                       # iterates would widen it
                assert np.all(np.max(np.abs(x - x64), axis=1)[both] <= tol)


# ---------------------------------------------------------------- 9, 10: failures
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.EDGE_NS)
def test_an_indefinite_matrix_at_every_pivot_position_and_nothing_lingers(oracle, n, dtype):
    """P[k][k] = -1 for k the first pivot, the last of the first 16-row block, the first of the second, the middle, the last
    two: numericError (the oracle's too: CPU tier), and the call right after it returns the family problem's bits."""
    P, q, l, u = fam(n, dtype)
    clean = device_family(n, dtype)
    for k in B.indefinite_positions(n):
        for p in range(COUNT):
            st, _, _ = M.solveBoxQP(B.lower_only(B.indefinite(P[p], k)), q[p], l[p], u[p], dtype=dtype)
            assert st == M.BoxQPStatus.numericError, (k, p)
            after = solve_single(P[p:p + 1], q[p:p + 1], l[p:p + 1], u[p:p + 1], dtype)
            assert same_bits(after, [a[p:p + 1] for a in clean]), (k, p)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.EDGE_NS)
def test_iteration_limit_and_nan(oracle, n, dtype):
    """maxIterations = 1: the problems that need more end with maxIterations after 1 step; a NaN in q[n - 1] makes every
    variable free in step 1 (no comparison with a NaN holds), the loop's `s == n` exit (quirk Q8): maxIterations after 1 step."""
    P, q, l, u = fam(n, dtype)
    scr = screen(oracle, n, dtype)
    s = M.BoxQPSettings(dtype); s.maxIterations = 1
    st, x, it = solve_single(P, q, l, u, dtype, settings=s)
    so, xo, io = B.oracle_solve(oracle, P, q, l, u, dtype, settings=B.qp_settings(oracle, dtype, maxIterations=1))
    assert np.array_equal(st[scr], so[scr]) and np.array_equal(it[scr], io[scr]) and np.all(it <= 1)
    assert np.any(so[scr] == M.BoxQPStatus.maxIterations)
    qn = q.copy(); qn[:, n - 1] = np.nan
    st, x, it = solve_single(P, qn, l, u, dtype)
    so, xo, io = B.oracle_solve(oracle, P, qn, l, u, dtype)
    assert np.all(so == M.BoxQPStatus.maxIterations) and np.all(io == 1)
    assert np.array_equal(st[scr], so[scr]) and np.array_equal(it[scr], io[scr]) and np.all(it <= 1)
