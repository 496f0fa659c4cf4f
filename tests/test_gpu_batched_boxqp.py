"""Batched box-constrained QP solves on the device (M.solveBoxQPBatched -> mir_lsq_batched_box_qp_s / _d -> k_boxqp_rows,
csrc/boxqp_rows.h: four problems a wave) against oracle.solve_box_qp, problem by problem, in both precisions.

What is compared, and to what:
  * status equals the oracle's of the same precision; on margin-screened problems (tests/boxqp_cases.py) so do the iteration
    count and the active set. The float oracle's ?posvx is unfused and the device's is fused, so x agrees to rounding only.
  * for status 0 an independent KKT check in numpy float64 on the device's x: l <= x <= u exactly, (Px + q)_i >= -tau_i at a
    lower bound, <= tau_i at an upper bound, |.| <= tau_i for a free variable, tau_i = 8 eps(T) (|P||x| + |q|)_i: the
    refinement stops at a componentwise backward error of eps, the factor 8 covers un-equilibration and the rounding of the
    compensated right-hand side. The same-precision oracle's own x needs a factor below 1 on these families
    (tests/test_batched_boxqp_host.py asserts <= 8 on the CPU), so 8 stands.
  * distance to the f64 oracle (on the same, rounded, data): double max|x - x64| <= 8 eps cond_2(P) max|x|; float 4 x the
    largest distance the float oracle itself shows from the f64 oracle over the family (computed here and printed), with the
    floor 4 eps max|x|.
  * mixed waves: problems of 0, 1, 2 and >= 3 iterations share a wave, in every rotation, and each must come back bit for bit
    as when it is solved alone -- the test of the group-divergence logic.
"""
import numpy as np
import pytest

import mir_optim_amd as M
import boxqp_cases as B
from boxqp_cases import check_against_oracle, same_bits, solve, x_tolerance

pytestmark = pytest.mark.gpu

DT = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


# ---------------------------------------------------------------- the random bounded family
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
@pytest.mark.parametrize("count", B.COUNTS)
def test_random_family_matches_the_oracle(oracle, n, dtype, count):
    """64 problems an order; a launch of `count` takes them cyclically (1, 3, 5, 7: a short last wave that repeats the last
    problem; 257: 65 waves, every problem of the family at least four times, in every group position)."""
    data = B.family(n, dtype)
    idx = np.arange(count) % B.FAMILY_COUNT
    dev = solve(*(a[idx] for a in data), dtype)
    check_against_oracle(dev, B.oracle_family(oracle, n, dtype), B.oracle_family(oracle, n, np.float64, dtype), data, dtype,
                         B.screen_family(oracle, n, dtype), idx)


@pytest.mark.parametrize("dtype", DT)
def test_grid_stride_repeats_the_small_launch_bit_for_bit(dtype):
    """More problems than the grid has groups (8192 waves of four): the waves stride over the rest. 32773 = 4 x 8192 + 5 problems
    of order 8, the family taken cyclically, must equal the 64-problem launch bit for bit."""
    data = B.family(8, dtype)
    ref = solve(*data, dtype)
    idx = np.arange(4 * 8192 + 5) % B.FAMILY_COUNT
    big = solve(*(a[idx] for a in data), dtype)
    assert same_bits(big, [a[idx] for a in ref])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
@pytest.mark.parametrize("rel", ["16eps", 1e-6])
@pytest.mark.parametrize("ab", ["16eps", 1e-6])
def test_non_default_classification_tolerances(oracle, n, dtype, rel, ab):
    eps = float(np.finfo(dtype).eps)
    rel, ab = (16 * eps if v == "16eps" else v for v in (rel, ab))
    data = B.family(n, dtype)
    so = B.qp_settings(oracle, dtype, relTolerance=rel, absTolerance=ab)
    s = M.BoxQPSettings(dtype); s.relTolerance = rel; s.absTolerance = ab
    dev = solve(*data, dtype, settings=s)
    ora = B.oracle_solve(oracle, *data, dtype, settings=so)
    ora64 = B.oracle_solve(oracle, *data, np.float64, settings=B.qp_settings(oracle, np.float64, relTolerance=rel, absTolerance=ab))
    check_against_oracle(dev, ora, ora64, data, dtype, B.screen_family(oracle, n, dtype))


# ---------------------------------------------------------------- mixed waves: the group-divergence logic
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
def test_mixed_waves_return_every_problem_as_when_solved_alone(oracle, n, dtype):
    found = B.mixed_wave(oracle, n, dtype)
    classes = sorted(found)
    assert classes == ([0, 1] if n == 1 else [0, 1, 2, 3])             # n = 1: boxqp_cases.mixed_wave says why
    wave = [found[classes[k % len(classes)]] for k in range(4)]
    P, q, l, u = (np.stack([w[k] for w in wave]) for k in range(4))
    alone = [solve(P[k:k + 1], q[k:k + 1], l[k:k + 1], u[k:k + 1], dtype) for k in range(4)]
    for k in range(4):
        st, x, it = alone[k]
        so, xo, io = oracle.solve_box_qp(np.tril(P[k]), q[k], l[k], u[k], dtype=dtype)
        assert st[0] == so == 0 and it[0] == io and min(io, 3) == classes[k % len(classes)]
        assert np.array_equal(B.active_set(x[0], l[k], u[k]), B.active_set(xo, l[k], u[k]))
    for rot in range(4):
        order = np.roll(np.arange(4), rot)
        got = solve(P[order], q[order], l[order], u[order], dtype)
        for pos, k in enumerate(order):
            assert same_bits([a[pos:pos + 1] for a in got], alone[k]), (rot, pos, k)


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
def test_no_bound_active_and_all_bounds_infinite(oracle, n, dtype):
    P, q, l, u = B.family(n, dtype)
    inf = np.full(n, np.inf)
    free = solve(P, q, -inf, inf, dtype)
    wide = solve(P, q, np.full(n, -1e3), np.full(n, 1e3), dtype)
    assert np.all(free[0] == 0) and np.all(free[2] == 0) and same_bits(free, wide)
    ora = B.oracle_solve(oracle, P, q, -inf, inf, dtype)
    ora64 = B.oracle_solve(oracle, P, q, -inf, inf, np.float64)
    assert np.all(ora[0] == 0) and np.all(ora[2] == 0)
    L, U = np.tile(-inf, (len(q), 1)), np.tile(inf, (len(q), 1))
    check_against_oracle(free, ora, ora64, (P, q, L, U), dtype, np.ones(len(q), bool))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
def test_every_bound_active_takes_the_path_without_a_solve(oracle, n, dtype):
    """P with positive entries, a corner z and multipliers g = P d > 0 (d > 0): q = g - P z puts the unconstrained minimiser
    z - d below l = z in every component, step 1 moves every variable to its lower bound (sN = 0: no reduced system), the
    multipliers are g and the loop ends: 1 iteration, x == l exactly."""
    rng = np.random.default_rng([11, n])
    Ps, qs, ls = [], [], []
    while len(Ps) < 16:
        A = np.abs(rng.standard_normal((n + 4, n)))
        P = (A.T @ A / (n + 4) + 0.05 * np.eye(n)).astype(dtype).astype(np.float64)
        if B.cond2(P) > 1e3:
            continue
        z, d = rng.standard_normal(n), rng.uniform(0.5, 2.0, n)
        Ps.append(P); qs.append((P @ d - P @ z).astype(dtype).astype(np.float64)); ls.append(z.astype(dtype).astype(np.float64))
    P, q, l = np.stack(Ps), np.stack(qs), np.stack(ls)
    u = l + 1
    st, x, it = solve(P, q, l, u, dtype)
    so, xo, io = B.oracle_solve(oracle, P, q, l, u, dtype)
    assert np.all(so == 0) and np.all(io == 1) and np.array_equal(xo, l)           # the construction does what it says
    assert np.array_equal(st, so) and np.array_equal(it, io) and np.array_equal(x.astype(np.float64), l)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
def test_equal_bounds(oracle, n, dtype):
    """l == u in every component (x is the bound, whatever the multipliers' signs), and in the even components only."""
    P, q, l, u = B.family(n, dtype)
    c = np.where(np.isfinite(l) & np.isfinite(u), (np.nan_to_num(l) + np.nan_to_num(u)) / 2, 0.25).astype(dtype).astype(np.float64)
    for fixed in (np.ones(n, bool), np.arange(n) % 2 == 0):
        lf, uf = np.where(fixed, c, l), np.where(fixed, c, u)
        st, x, it = solve(P, q, lf, uf, dtype)
        so, xo, io = B.oracle_solve(oracle, P, q, lf, uf, dtype)
        assert np.array_equal(st, so)
        ok = st == 0
        assert np.array_equal(x.astype(np.float64)[ok][:, fixed], c[ok][:, fixed])
        if fixed.all():
            assert np.array_equal(it, io) and np.array_equal(x.astype(np.float64)[ok], xo[ok])
        else:
            s64, x64, _ = B.oracle_solve(oracle, P, q, lf, uf, np.float64)
            both = ok & (s64 == 0)
            tol = x_tolerance(dtype, P, x64, xo)
            assert np.all(np.max(np.abs(x - x64), axis=1)[both] <= tol[both])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
def test_shared_bounds_and_per_problem_bounds_give_identical_bits(n, dtype):
    P, q, _, _ = B.family(n, dtype)
    l, u = np.full(n, -0.5), np.linspace(0.25, 0.75, n)
    shared = solve(P, q, l, u, dtype)
    each = solve(P, q, np.tile(l, (len(q), 1)), np.tile(u, (len(q), 1)), dtype)
    assert same_bits(shared, each) and np.any(shared[2] > 0)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
def test_handing_in_the_unconstrained_solution(oracle, n, dtype):
    """MIR_LSQ_BOX_QP_UNCONSTRAINED_SOLUTION with x = the oracle's unconstrained solution in the same precision: status, active
    set and iterations as without the flag (exact on margin-screened problems), x within the tolerances of this file; and the
    oracle called the same way agrees."""
    data = B.family(n, dtype)
    P, q, l, u = data
    inf = np.full(n, np.inf)
    s0, x0, _ = B.oracle_solve(oracle, P, q, -inf, inf, dtype)
    assert np.all(s0 == 0)
    plain = solve(*data, dtype)
    given = solve(*data, dtype, x=x0, unconstrainedSolution=True)
    scr = B.screen_family(oracle, n, dtype)
    assert np.array_equal(given[0], plain[0]) and np.array_equal(given[2][scr], plain[2][scr])
    assert np.array_equal(B.active_set(given[1], l, u)[scr], B.active_set(plain[1], l, u)[scr])
    ora = B.oracle_solve(oracle, *data, dtype, x0=x0)
    check_against_oracle(given, ora, B.oracle_family(oracle, n, np.float64, dtype), data, dtype, scr)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
def test_an_indefinite_problem_fails_alone(oracle, n, dtype):
    """numericError for the indefinite problem, in every group position, and the three problems that share its wave come back
    as in a wave without it, bit for bit."""
    P, q, l, u = (a[:4].copy() for a in B.family(n, dtype))
    clean = solve(P, q, l, u, dtype)
    for pos in range(4):
        Pb = P.copy()
        Pb[pos] = -np.eye(n) if n < 3 else np.diag(np.where(np.arange(n) == n - 2, -1.0, 1.0))
        so = oracle.solve_box_qp(np.tril(Pb[pos]), q[pos], l[pos], u[pos], dtype=dtype)[0]
        got = solve(Pb, q, l, u, dtype)
        assert got[0][pos] == so == M.BoxQPStatus.numericError
        others = np.arange(4) != pos
        assert same_bits([a[others] for a in got], [a[others] for a in clean])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", B.NS)
def test_iteration_limit_and_nan(oracle, n, dtype):
    """qpSettings.maxIterations = 1 on the family: the problems that need more end with maxIterations after 1 step, the others
    are untouched; a NaN in q makes every variable free in step 1 (no comparison with a NaN holds), which is the loop's
    `s == n` exit (quirk Q8): maxIterations after 1 step, as the oracle reports it -- and the wave's other problems do not care."""
    data = B.family(n, dtype)
    P, q, l, u = data
    s = M.BoxQPSettings(dtype); s.maxIterations = 1
    st, x, it = solve(*data, dtype, settings=s)
    so, xo, io = B.oracle_solve(oracle, *data, dtype, settings=B.qp_settings(oracle, dtype, maxIterations=1))
    scr = B.screen_family(oracle, n, dtype)
    assert np.array_equal(st[scr], so[scr]) and np.array_equal(it[scr], io[scr]) and np.all(it <= 1)
    if n > 1:
        assert np.any(so[scr] == M.BoxQPStatus.maxIterations)
    full = solve(*data, dtype)
    qn = q.copy()
    qn[1::4, n - 1] = np.nan
    got = solve(P, qn, l, u, dtype)
    for p in range(1, len(q), 4):
        so1, _, io1 = oracle.solve_box_qp(np.tril(P[p]), qn[p], l[p], u[p], dtype=dtype)
        assert (got[0][p], got[2][p]) == (so1, io1) == (M.BoxQPStatus.maxIterations, 1)
    others = np.arange(len(q)) % 4 != 1
    assert same_bits([a[others] for a in got], [a[others] for a in full])
