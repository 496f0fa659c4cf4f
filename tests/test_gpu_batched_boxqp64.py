"""Batched box-constrained QP solves of order 17 .. 64 on the device (M.solveBoxQPBatchedWide -> mir_lsq_batched_box_qp64_s /
_d -> k_boxqp_wave<W, T>, csrc/boxqp_wave.h: one problem a wave at W = 64, two at W = 32, the matrices in LDS, the order a
run-time argument) against oracle.solve_box_qp, problem by problem, in both precisions. Orders: 17, 31, 32 (W = 32) and 33, 63,
64 (W = 64) -- for each instance the first, one short of full, and full. 64 problems an order (boxqp_cases.family), P handed in
as its lower triangle with NaN above (QP:109).

The comparison rules are those of the other box QP device tests, through the same boxqp_cases.check_against_oracle:
  * status equals the same-precision oracle's; on margin-screened problems so do the iteration count and the active set. The
    screen is boxqp_cases.SINGLE_MARGIN (float 3e-5, double 1e-8); tests/test_batched_boxqp64_host.py keeps on the CPU that it
    drops at most 2 of 64 problems and that the float oracle takes the f64 oracle's path on the rest;
  * an independent KKT check of the device's x in numpy float64 with the factor 8;
  * distance to the f64 oracle on the same (rounded) data: double 8 eps cond_2(P) max|x|; float 4 x the float oracle's own
    largest distance, floor 4 eps max|x|.
Independence, bit for bit: a second call; one wave solving the whole family in sequence (max_waves = 1) against the default
grid, also with an indefinite, a NaN and an out-of-iterations problem in the sequence; the grid-stride loop; every ordered pair
of a 0, 1, 2 and >= 3 step problem in the two halves of a W = 32 wave; a reversed batch at W = 64.
Beyond the family, as tests/test_gpu_boxqp_single.py: non-default classification tolerances, unconstrainedSolution = true,
infinite bounds against a box of +-1e3, float ?posvx on badly scaled rows, every bound active, l == u, an indefinite P,
maxIterations = 1, a NaN in q (quirk Q8); shared against per-problem bounds; a decoupled 17th variable on family(16) against
the n = 16 kernel.

Measured on an MI355X with this file (worst over the orders of an instance, 64 problems each; KKT factor needed / largest
distance over its tolerance):
  instance (orders run)              float32          float64
  k_boxqp_wave<32> (17, 31, 32)      0.76 / 0.422     0.88 / 0.009
  k_boxqp_wave<64> (33, 63, 64)      0.87 / 0.385     1.12 / 0.004
Badly scaled float rows (test_float_posvx_on_badly_scaled_rows): the device's largest relative error 3.2e-7 .. 1.7e-6 over the
six orders, the float oracle's 3.4e-7 .. 1.8e-6; the device's largest over the oracle's largest at most 1.34 (n = 33).
"""
import functools

import numpy as np
import pytest

import mir_optim_amd as M
import boxqp_cases as B
import boxqp64_cases as B64
from boxqp_cases import check_against_oracle, same_bits, x_tolerance
from boxqp64_cases import COUNT, NS64, NS_W32, NS_W64, fam, oracles, screen, solve

pytestmark = pytest.mark.gpu

DT = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
_DEVICE = {}


def device_family(n, dtype):
    """the device's answers on the family with default settings and the default grid, computed once and shared (read-only)"""
    key = (n, np.dtype(dtype).name)
    if key not in _DEVICE:
        res = solve(*fam(n, dtype), dtype)
        for a in res:
            a.setflags(write=False)
        _DEVICE[key] = res
    return _DEVICE[key]


def take(res, idx):
    return [a[idx] for a in res]


# ---------------------------------------------------------------- 1, 2: the family, and the same bits from a second call
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_family_matches_the_oracle(oracle, n, dtype):
    """counts 1, 2, 3, 64 and 129, the family taken cyclically: a short last wave at W = 32 (1, 3, 129), every problem in both
    halves (129 shifts the pairing)"""
    data = fam(n, dtype)
    ora, ora64 = oracles(oracle, n, dtype)
    scr = screen(oracle, n, dtype)
    dev = device_family(n, dtype)
    kkt, ratio = B.worst_figures(dev, ora, ora64, data, dtype)
    print(f"k_boxqp_wave<{32 if n <= 32 else 64}> {np.dtype(dtype).name} n = {n}: KKT factor {kkt:.2f}, distance / tolerance {ratio:.4f}, "
          f"iterations {dev[2].min()} .. {dev[2].max()}")
    check_against_oracle(dev, ora, ora64, data, dtype, scr)
    for count in (1, 2, 3, 129):
        idx = np.arange(count) % COUNT
        got = solve(*take(data, idx), dtype)
        check_against_oracle(got, ora, ora64, data, dtype, scr, idx)
        assert same_bits(got, take(dev, idx)), count


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_a_second_call_gives_the_same_bits(n, dtype):
    first = device_family(n, dtype)
    again = solve(*fam(n, dtype), dtype)
    assert same_bits(again, first)


# ---------------------------------------------------------------- 3: one wave solves the batch in sequence
@functools.lru_cache(maxsize=None)
def out_of_iterations_problem(oracle, n, dtype):
    """the first family problem whose l == u version (boxqp_cases.equal_bounds_centre) makes the oracle's loop cycle to its
    default limit of 10 n + 100 steps"""
    P, q, l, u = fam(n, dtype)
    c = B.equal_bounds_centre(l, u, dtype)
    for p in range(COUNT):
        st, _, it = oracle.solve_box_qp(np.tril(P[p]), q[p], c[p], c[p], dtype=dtype)
        if st == M.BoxQPStatus.maxIterations:
            assert it == 10 * n + 100
            return P[p], q[p], c[p], c[p]
    raise AssertionError("no l == u problem of the family runs out of iterations")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_one_wave_in_sequence_equals_the_default_grid(oracle, n, dtype):
    """max_waves = 1: one wave takes all 64 problems (32 pairs at W = 32) one after the other through the same LDS. The same with
    an indefinite problem, a NaN-in-q problem and a problem that runs out of iterations at positions 0, 1 and 31, in every
    assignment of the three to those positions' rotation: each answers as the oracle says and the untouched problems keep their
    bits -- nothing lingers in LDS or in a register."""
    data = fam(n, dtype)
    clean = device_family(n, dtype)
    assert same_bits(solve(*data, dtype, max_waves=1), clean)
    P, q, l, u = (a.copy() for a in data)
    Pm, qm, lm, um = out_of_iterations_problem(oracle, n, dtype)
    spots = (0, 1, COUNT // 2 - 1)
    for rot in range(3):
        Pb, qb, lb, ub = P.copy(), q.copy(), l.copy(), u.copy()
        bad, nan, lim = (spots[(rot + k) % 3] for k in range(3))
        Pb[bad] = B.indefinite(P[bad], n // 2)
        qb[nan, n - 1] = np.nan
        Pb[lim], qb[lim], lb[lim], ub[lim] = Pm, qm, lm, um
        for waves in (1, 0):
            st, x, it = got = solve(Pb, qb, lb, ub, dtype, max_waves=waves)
            assert st[bad] == M.BoxQPStatus.numericError
            assert (st[nan], it[nan]) == (M.BoxQPStatus.maxIterations, 1)
            assert (st[lim], it[lim]) == (M.BoxQPStatus.maxIterations, 10 * n + 100)
            others = ~np.isin(np.arange(COUNT), spots)
            assert same_bits(take(got, others), take(clean, others)), (rot, waves)


# ---------------------------------------------------------------- 4: the grid-stride loop
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", [17, 33])
def test_grid_stride_repeats_the_small_launch_bit_for_bit(n, dtype):
    """More problems than the grid has places (8192 waves of two problems at n = 17, of one at n = 33): the waves stride over
    the rest. (problems a wave) x 8192 + 5 problems, the family taken cyclically, must equal the 64-problem launch."""
    data = fam(n, dtype)
    ref = device_family(n, dtype)
    idx = np.arange(B64.problems_per_wave(n) * B64.GRID_WAVES + 5) % COUNT
    big = solve(*take(data, idx), dtype)
    assert same_bits(big, take(ref, idx))


# ---------------------------------------------------------------- 5, 6: who shares a wave, and who came before
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS_W32)
def test_every_ordered_pair_of_a_mixed_wave_returns_each_problem_as_when_solved_alone(oracle, n, dtype):
    found = dict(B.mixed_wave(oracle, n, dtype))
    assert sorted(found) == [1, 2, 3]
    found[0] = B64.class0(found, n)
    classes = [0, 1, 2, 3]
    P, q, l, u = (np.stack([found[c][k] for c in classes]) for k in range(4))
    alone = [solve(P[k:k + 1], q[k:k + 1], l[k:k + 1], u[k:k + 1], dtype) for k in range(4)]
    for k in range(4):
        st, x, it = alone[k]
        so, xo, io = oracle.solve_box_qp(np.tril(P[k]), q[k], l[k], u[k], dtype=dtype)
        assert st[0] == so == 0 and it[0] == io and min(io, 3) == classes[k]
        assert np.array_equal(B.active_set(x[0], l[k], u[k]), B.active_set(xo, l[k], u[k]))
    pairs = np.array([(a, b) for a in range(4) for b in range(4)]).reshape(-1)      # problems 2 k and 2 k + 1 share a wave
    got = solve(P[pairs], q[pairs], l[pairs], u[pairs], dtype)
    for pos, k in enumerate(pairs):
        assert same_bits([a[pos:pos + 1] for a in got], alone[k]), (pos, k)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS_W64)
def test_a_reversed_batch_returns_each_problems_bits(n, dtype):
    """W = 64: a wave's previous problem is another one in the reversed batch, with the default grid and with three waves"""
    data = fam(n, dtype)
    clean = device_family(n, dtype)
    rev = np.arange(COUNT)[::-1]
    for waves in (0, 3):
        assert same_bits(solve(*take(data, rev), dtype, max_waves=waves), take(clean, rev)), waves


# ---------------------------------------------------------------- 7: the cases of tests/test_gpu_boxqp_single.py
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
@pytest.mark.parametrize("rel", ["16eps", 1e-6])
@pytest.mark.parametrize("ab", ["16eps", 1e-6])
def test_non_default_classification_tolerances(oracle, n, dtype, rel, ab):
    eps = float(np.finfo(dtype).eps)
    rel, ab = (16 * eps if v == "16eps" else v for v in (rel, ab))
    data = fam(n, dtype)
    s = M.BoxQPSettings(dtype); s.relTolerance = rel; s.absTolerance = ab
    dev = solve(*data, dtype, settings=s)
    ora = B.oracle_solve(oracle, *data, dtype, settings=B.qp_settings(oracle, dtype, relTolerance=rel, absTolerance=ab))
    ora64 = B.oracle_solve(oracle, *data, np.float64, settings=B.qp_settings(oracle, np.float64, relTolerance=rel, absTolerance=ab))
    check_against_oracle(dev, ora, ora64, data, dtype, screen(oracle, n, dtype))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_handing_in_the_unconstrained_solution(oracle, n, dtype):
    """unconstrainedSolution = true with x = the same-precision oracle's unconstrained solution: status and, on screened problems,
    iterations and active set as without the flag; and the oracle called the same way agrees."""
    data = fam(n, dtype)
    P, q, l, u = data
    inf = np.full(n, np.inf)
    s0, x0, _ = B.oracle_solve(oracle, P, q, -inf, inf, dtype)
    assert np.all(s0 == 0)
    plain = device_family(n, dtype)
    given = solve(*data, dtype, x=x0, unconstrainedSolution=True)
    scr = screen(oracle, n, dtype)
    assert np.array_equal(given[0], plain[0]) and np.array_equal(given[2][scr], plain[2][scr])
    assert np.array_equal(B.active_set(given[1], l, u)[scr], B.active_set(plain[1], l, u)[scr])
    ora = B.oracle_solve(oracle, *data, dtype, x0=x0)
    check_against_oracle(given, ora, oracles(oracle, n, dtype)[1], data, dtype, scr)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_infinite_bounds_and_a_huge_box(oracle, n, dtype):
    """status 0 and 0 iterations, x by the distance rule against oracle.posvx's solution (the KKT check with it), and the bits of
    the same problem inside a box of +-1e3"""
    P, q, _, _ = fam(n, dtype)
    inf = np.full(n, np.inf)
    free = solve(P, q, -inf, inf, dtype)
    wide = solve(P, q, np.full(n, -1e3), np.full(n, 1e3), dtype)
    assert np.all(free[0] == 0) and np.all(free[2] == 0) and same_bits(free, wide)
    zero = np.zeros(COUNT, dtype=np.int32)
    sols = [[oracle.posvx(P[p], -q[p], dt) for p in range(COUNT)] for dt in (dtype, np.float64)]
    assert all(r["info"] == 0 for rs in sols for r in rs)
    ora, ora64 = ((zero, np.stack([r["x"] for r in rs]).astype(np.float64), zero) for rs in sols)
    L, U = np.tile(-inf, (COUNT, 1)), np.tile(inf, (COUNT, 1))
    check_against_oracle(free, ora, ora64, (P, q, L, U), dtype, np.ones(COUNT, bool))


@pytest.mark.parametrize("n", NS64)
def test_float_posvx_on_badly_scaled_rows(oracle, n):
    """D P D with D = 10^U(-1.5, 1.5) in float32 (equilibration must act), infinite bounds; the rule of
    tests/test_gpu_boxqp_single.py: against x*, the refined float64 solution of the rounded system, the device's error is at most
    10 x the float oracle's + eps32, and the two differ by at most 4 max(err, err_oracle) + eps32 (relative 2-norms)."""
    P, q = B.badly_scaled_family(n)
    count = len(q)
    inf = np.full(n, np.inf)
    eps = float(np.finfo(np.float32).eps)
    st, x, it = solve(P, q, -inf, inf, np.float32)
    so, xo, io = B.oracle_solve(oracle, P, q, -inf, inf, np.float32)
    assert np.all(st == 0) and np.all(so == 0) and np.all(it == 0) and np.all(io == 0)
    x = x.astype(np.float64)
    worst = [0.0, 0.0]
    for p in range(count):
        xr = B.refined_solve(P[p], -q[p])
        err = np.linalg.norm(x[p] - xr) / np.linalg.norm(xr)
        erro = np.linalg.norm(xo[p] - xr) / np.linalg.norm(xr)
        worst = [max(worst[0], err), max(worst[1], erro)]
        assert err <= 10 * erro + eps, (p, err, erro)
        assert np.linalg.norm(x[p] - xo[p]) / np.linalg.norm(xo[p]) <= 4 * max(err, erro) + eps, (p, err, erro)
    print(f"n = {n}: largest relative error, device {worst[0]:.3e}, float oracle {worst[1]:.3e}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_every_bound_active_takes_the_path_without_a_solve(oracle, n, dtype):
    P, q, l, u, _ = B.all_active_family(n, dtype)
    st, x, it = solve(P, q, l, u, dtype)
    so, xo, io = B.oracle_solve(oracle, P, q, l, u, dtype)
    assert np.all(so == 0) and np.all(io == 1) and np.array_equal(xo, l)           # the construction does what it says
    assert np.array_equal(st, so) and np.array_equal(it, io) and np.array_equal(x.astype(np.float64), l)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_equal_bounds(oracle, n, dtype):
    """l == u in every component (x is the bound, whatever the multipliers' signs), and in the even components only, with
    maxIterations = 64 on both sides (boxqp_cases.EQUAL_BOUNDS_MAX_ITERATIONS: the reference's loop cycles on most of these
    problems). Where the status is maxIterations on both sides x, the last iterate, still has its fixed components on the bound."""
    P, q, l, u = fam(n, dtype)
    c = B.equal_bounds_centre(l, u, dtype)
    s = M.BoxQPSettings(dtype); s.maxIterations = B.EQUAL_BOUNDS_MAX_ITERATIONS
    so_ = lambda dt: B.qp_settings(oracle, dt, maxIterations=B.EQUAL_BOUNDS_MAX_ITERATIONS)
    for fixed in (np.ones(n, bool), np.arange(n) % 2 == 0):
        lf, uf = np.where(fixed, c, l), np.where(fixed, c, u)
        st, x, it = solve(P, q, lf, uf, dtype, settings=s)
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


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_an_indefinite_matrix_at_every_pivot_position(oracle, n, dtype):
    """P[k][k] = -1 for k the first pivot, the last of the first 16 rows, the first of the next, the middle, the last two, in
    every second problem of the batch: numericError (the oracle's too: CPU tier), and the problems between them keep their bits."""
    P, q, l, u = fam(n, dtype)
    clean = device_family(n, dtype)
    bad = np.arange(COUNT) % 2 == 1
    for k in B.indefinite_positions(n):
        Pb = P.copy()
        Pb[bad, k, k] = -1.0
        got = solve(Pb, q, l, u, dtype)
        assert np.all(got[0][bad] == M.BoxQPStatus.numericError), k
        assert same_bits(take(got, ~bad), take(clean, ~bad)), k
        got = solve(Pb[bad], q[bad], l[bad], u[bad], dtype)                       # and with nobody else in the wave
        assert np.all(got[0] == M.BoxQPStatus.numericError), k


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_iteration_limit_and_nan(oracle, n, dtype):
    """maxIterations = 1: the problems that need more end with maxIterations after 1 step; a NaN in q[n - 1] makes every
    variable free in step 1 (no comparison with a NaN holds), the loop's `s == n` exit (quirk Q8): maxIterations after 1 step."""
    P, q, l, u = fam(n, dtype)
    scr = screen(oracle, n, dtype)
    s = M.BoxQPSettings(dtype); s.maxIterations = 1
    st, x, it = solve(P, q, l, u, dtype, settings=s)
    so, xo, io = B.oracle_solve(oracle, P, q, l, u, dtype, settings=B.qp_settings(oracle, dtype, maxIterations=1))
    assert np.array_equal(st[scr], so[scr]) and np.array_equal(it[scr], io[scr]) and np.all(it <= 1)
    assert np.any(so[scr] == M.BoxQPStatus.maxIterations)
    qn = q.copy(); qn[:, n - 1] = np.nan
    st, x, it = solve(P, qn, l, u, dtype)
    so, xo, io = B.oracle_solve(oracle, P, qn, l, u, dtype)
    assert np.all(so == M.BoxQPStatus.maxIterations) and np.all(io == 1)
    assert np.array_equal(st[scr], so[scr]) and np.array_equal(it[scr], io[scr]) and np.all(it <= 1)


# ---------------------------------------------------------------- 8: shared and per-problem bounds
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", NS64)
def test_shared_bounds_and_per_problem_bounds_give_identical_bits(n, dtype):
    P, q, _, _ = fam(n, dtype)
    l, u = np.full(n, -0.5), np.linspace(0.25, 0.75, n)
    shared = solve(P, q, l, u, dtype)
    each = solve(P, q, np.tile(l, (len(q), 1)), np.tile(u, (len(q), 1)), dtype)
    assert same_bits(shared, each) and np.any(shared[2] > 0)


# ---------------------------------------------------------------- 9: consistency with the n <= 16 kernel
@pytest.mark.parametrize("dtype", DT)
def test_a_decoupled_17th_variable_leaves_the_n16_problem_as_the_n16_kernel_solves_it(oracle, dtype):
    """family(16) with a 17th, decoupled variable (P[16][16] = 1, q[16] = 0, bounds +-1e3: its minimiser 0 is free) through the
    wave kernel at n = 17: status equal on every problem, iteration count and active set of the first sixteen variables those of
    the n = 16 kernel on the problems that pass the 1e-3 screen of family(16), x[:, 16] == 0 and x[:, :16] within this file's
    distance of the f64 oracle. Equilibration sees one more diagonal entry and the sums run in another order, so bits are not
    demanded."""
    P16, q16, l16, u16 = B.family(16, dtype)
    count = len(q16)
    P = np.zeros((count, 17, 17)); P[:, :16, :16] = P16; P[:, 16, 16] = 1.0
    q = np.concatenate([q16, np.zeros((count, 1))], axis=1)
    l = np.concatenate([l16, np.full((count, 1), -1e3)], axis=1)
    u = np.concatenate([u16, np.full((count, 1), 1e3)], axis=1)
    st17, x17, it17 = solve(P, q, l, u, dtype)
    st16, x16, it16 = B.solve(P16, q16, l16, u16, dtype)
    scr = B.screen_family(oracle, 16, dtype)
    assert np.array_equal(st17, st16) and np.array_equal(it17[scr], it16[scr])
    assert np.array_equal(B.active_set(x17[:, :16], l16, u16)[scr], B.active_set(x16, l16, u16)[scr])
    assert np.all(x17[:, 16] == 0)
    so, xo, _ = B.oracle_family(oracle, 16, dtype)
    s64, x64, _ = B.oracle_family(oracle, 16, np.float64, dtype)
    both = (st17 == 0) & (s64 == 0)
    tol = x_tolerance(dtype, P16, x64, xo)
    dist = np.max(np.abs(x17[:, :16].astype(np.float64) - x64), axis=1)
    print(f"largest distance from the f64 oracle: {np.max(dist[both], initial=0):.3e}")
    assert np.all(dist[both] <= tol[both]), (dist[both] / tol[both]).max()
