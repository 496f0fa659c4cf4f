"""The one-problem BOXCQP entry (mir_solve_box_qp_gpu_s / _d, M.solveBoxQP), CPU tier: what tests/test_gpu_boxqp_single.py relies
on, kept by the oracle alone, at every order of boxqp_cases.NS_SINGLE (both sides of every edge between the entry's kernel
classes, one short of a full 16-row block, 1, 2 and 300) and in both precisions, on family(n, dtype, count=16):

  * conditioning (cond_2 <= 1e3), status 0 on all 16, at least 2 active-set iterations on every problem from n = 15 on;
  * at most 2 of 16 problems fail the margin screen at SINGLE_MARGIN (float 3e-5, double 1e-8);
  * the float oracle takes the f64 oracle's path (iteration count, active set) on every screened problem;
  * the oracle's own x passes the KKT check with a factor <= 8;
  * the f64 distance bar 8 eps cond_2(P) max|x| is not vacuous: the f64 oracle's x lies within a quarter of it of the
    extended-precision solution on its own final active set (the reduced system solved in numpy float64 and refined in long
    double), so the bar leaves the device no more than the reference's class of error times a known factor;
  * the constructions of the device edge tests do what they say: every bound active (status 0, 1 iteration, x == l), a NaN in
    q[n - 1] (maxIterations after 1 step, quirk Q8), maxIterations = 1, an indefinite P with the bad pivot at the first, a
    middle and the last positions (numericError), badly scaled float rows (solved), and |x| of the unconstrained minimiser far
    inside the box of +-1e3 that the device test compares infinite bounds with.

Measured with this file (the printed lines): screened out at most 2 of 16 (float, n = 256; 1 at n = 33, 127, 255; double none);
the oracle's worst KKT factor 1.37 (f64, n = 256); the f64 oracle uses 12.1 % of the distance bound at n = 1, 3.9 % at n = 2 and
at most 0.95 % from n = 15 on (n = 300, on the data rounded to float); 2 .. 7 iterations from n = 15 on.
"""
import numpy as np
import pytest

import boxqp_cases as B

PREC = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
COUNT = B.SINGLE_COUNT
STATUS_NUMERIC_ERROR, STATUS_MAX_ITERATIONS = 1, 2                                  # boxcqp.d:18-26


@pytest.mark.parametrize("dtype", PREC)
@pytest.mark.parametrize("n", B.NS_SINGLE)
def test_family_conditioning_status_and_screen(oracle, n, dtype):
    P, q, l, u = B.family(n, dtype, count=COUNT)
    assert P.shape == (COUNT, n, n) and all(B.cond2(Pp) <= 1e3 for Pp in P) and np.all(l < u)
    st, x, it = B.oracle_family(oracle, n, dtype, count=COUNT)
    st64, x64, it64 = B.oracle_family(oracle, n, np.float64, dtype, COUNT)
    assert np.all(st == 0) and np.all(st64 == 0)
    if n >= 15:
        assert it.min() >= 2 and it64.min() >= 2, (it, it64)
    keep = B.screen_family(oracle, n, dtype, B.SINGLE_MARGIN[dtype], COUNT)
    out = COUNT - int(keep.sum())
    print(f"n = {n} {np.dtype(dtype).name}: {out} of {COUNT} screened out at margin {B.SINGLE_MARGIN[dtype]:g}; "
          f"iterations {it.min()} .. {it.max()}")
    assert out <= B.SINGLE_MAX_SCREENED_OUT
    assert np.array_equal(it[keep], it64[keep]) and np.array_equal(B.active_set(x, l, u)[keep], B.active_set(x64, l, u)[keep])


@pytest.mark.parametrize("dtype", PREC)
@pytest.mark.parametrize("n", B.NS_SINGLE)
def test_kkt_and_the_f64_distance_bar(oracle, n, dtype):
    """The same-precision oracle's KKT factor, and the share of x_tolerance(float64) that the f64 oracle itself uses on the same
    (rounded) data: at most a quarter (measured: the module docstring)."""
    P, q, l, u = B.family(n, dtype, count=COUNT)
    st, x, it = B.oracle_family(oracle, n, dtype, count=COUNT)
    need = max(B.kkt_factor(P[p], q[p], l[p], u[p], x[p], np.finfo(dtype).eps) for p in range(COUNT))
    st64, x64, _ = B.oracle_family(oracle, n, np.float64, dtype, COUNT)
    tol = B.x_tolerance(np.float64, P, x64, x64)
    xs = np.stack([B.solution_on_active_set(P[p], q[p], l[p], u[p], x64[p]) for p in range(COUNT)])
    share = float(np.max(np.max(np.abs(x64 - xs), axis=1) / tol))
    print(f"n = {n} {np.dtype(dtype).name}: the oracle needs a KKT factor of {need:.2f}; the f64 oracle uses {100 * share:.2f} % of the "
          f"f64 distance bound")
    assert need <= B.KKT_FACTOR
    assert share <= 0.25


@pytest.mark.parametrize("dtype", PREC)
@pytest.mark.parametrize("n", B.NS_SINGLE)
def test_every_bound_active_construction(oracle, n, dtype):
    P, q, l, u, draws = B.all_active_family(n, dtype)
    assert all(B.cond2(Pp) <= 1e3 for Pp in P) and draws <= 64 * COUNT
    assert all(np.array_equal(a.astype(dtype).astype(np.float64), a) for a in (P, q, l, u))
    so, xo, io = B.oracle_solve(oracle, P, q, l, u, dtype)
    print(f"n = {n} {np.dtype(dtype).name}: {draws} draws of d for {COUNT} problems")
    assert np.all(so == 0) and np.all(io == 1) and np.array_equal(xo, l)


@pytest.mark.parametrize("dtype", PREC)
@pytest.mark.parametrize("n", B.NS_SINGLE)
def test_nan_and_iteration_limit_constructions(oracle, n, dtype):
    P, q, l, u = B.family(n, dtype, count=COUNT)
    qn = q.copy(); qn[:, n - 1] = np.nan
    so, _, io = B.oracle_solve(oracle, P, qn, l, u, dtype)
    assert np.all(so == STATUS_MAX_ITERATIONS) and np.all(io == 1)                   # quirk Q8
    so, _, io = B.oracle_solve(oracle, P, q, l, u, dtype, settings=B.qp_settings(oracle, dtype, maxIterations=1))
    if n >= 15:
        assert np.all(so == STATUS_MAX_ITERATIONS) and np.all(io == 1)
    else:                                   # n = 1 ends in step 1 whenever a bound is violated (boxqp_cases.mixed_wave says why)
        seen = set(zip(so.tolist(), io.tolist()))
        assert seen == ({(0, 0), (0, 1)} if n == 1 else {(0, 0), (0, 1), (STATUS_MAX_ITERATIONS, 1)}), seen


@pytest.mark.parametrize("dtype", PREC)
@pytest.mark.parametrize("n", B.NS_SINGLE)
def test_indefinite_construction(oracle, n, dtype):
    P, q, l, u = B.family(n, dtype, count=COUNT)
    ks = B.indefinite_positions(n)
    assert ks[0] == 0 and ks[-1] == n - 1 and all(0 <= k < n for k in ks)
    for k in ks:
        d = np.ones(n); d[k] = -1.0
        assert oracle.solve_box_qp(np.diag(d), q[0], l[0], u[0], dtype=dtype)[0] == STATUS_NUMERIC_ERROR, k
        for p in range(COUNT):
            assert oracle.solve_box_qp(np.tril(B.indefinite(P[p], k)), q[p], l[p], u[p], dtype=dtype)[0] == STATUS_NUMERIC_ERROR, (k, p)


@pytest.mark.parametrize("n", B.EDGE_NS)
def test_unconstrained_constructions(oracle, n):
    """Infinite bounds: the minimiser lies far inside +-1e3 in both precisions (the device test asks for the bits of that box);
    the badly scaled float rows are solved by the float oracle to the accuracy of the well-scaled system (measured: a relative
    error of at most 1.8e-6), so ten times that error is a rule the device can be held to."""
    inf = np.full(n, np.inf)
    for dtype in B.DTYPES:
        P, q, _, _ = B.family(n, dtype, count=COUNT)
        so, xo, io = B.oracle_solve(oracle, P, q, -inf, inf, dtype)
        assert np.all(so == 0) and np.all(io == 0) and np.abs(xo).max() <= 100.0
        for p in range(COUNT):
            r = oracle.posvx(P[p], -q[p], dtype)
            assert r["info"] == 0 and np.array_equal(r["x"].astype(np.float64), xo[p])
    P, q = B.badly_scaled_family(n)
    so, xo, io = B.oracle_solve(oracle, P, q, -inf, inf, np.float32)
    assert np.all(so == 0) and np.all(io == 0)
    err = max(np.linalg.norm(xo[p] - xr) / np.linalg.norm(xr) for p in range(COUNT) for xr in [B.refined_solve(P[p], -q[p])])
    print(f"n = {n}: badly scaled float rows, the float oracle's largest relative error {err:.3e}")
    assert err <= 1e3 * np.finfo(np.float32).eps       # cond_2 <= 1e3 before the scaling that ?poequ takes out again, times eps


@pytest.mark.parametrize("dtype", PREC)
@pytest.mark.parametrize("n", B.EDGE_NS)
def test_equal_bounds_construction(oracle, n, dtype):
    """l == u in every component and in the even ones: the reference's loop ends on every problem at n = 2, on a few at n = 16
    and 17 (within 5 steps), on none from n = 64 on, where it cycles until maxIterations (10 n + 100 by default: 2.6 .. 5.6 s a
    case for the oracle alone at n = 256 and 257, measured). With EQUAL_BOUNDS_MAX_ITERATIONS the status is the same, the
    problems that end are untouched (asserted up to n = 65, where the default limit is quick), and the last iterate of a
    cycle still has its fixed components on the bound."""
    P, q, l, u = B.family(n, dtype, count=COUNT)
    c = B.equal_bounds_centre(l, u, dtype)
    lim = B.qp_settings(oracle, dtype, maxIterations=B.EQUAL_BOUNDS_MAX_ITERATIONS)
    for fixed in (np.ones(n, bool), np.arange(n) % 2 == 0):
        lf, uf = np.where(fixed, c, l), np.where(fixed, c, u)
        so, xo, io = B.oracle_solve(oracle, P, q, lf, uf, dtype, settings=lim)
        ok = so == 0
        print(f"n = {n} {np.dtype(dtype).name}, {'every' if fixed.all() else 'even'} component fixed: {int(ok.sum())} of {COUNT} solved")
        assert set(so.tolist()) <= {0, STATUS_MAX_ITERATIONS} and np.array_equal(xo[:, fixed], c[:, fixed])
        assert np.all(io[~ok] == B.EQUAL_BOUNDS_MAX_ITERATIONS) and np.all(io[ok] <= 8)
        assert ok.all() if n == 2 else (not ok.any() if n >= 64 else ok.any())
        if n <= 65:
            sd, xd, idd = B.oracle_solve(oracle, P, q, lf, uf, dtype)
            assert np.array_equal(sd, so) and np.array_equal(xd[ok], xo[ok]) and np.array_equal(idd[ok], io[ok])


def test_the_fuzz_case_that_float_rounding_decides(oracle):
    """scripts/fuzz_boxqp.py, seed 44 in float: n = 128 (k_box_qp<float, 8>, reached since the float cap went for benign shifts),
    cond_2 = 32, a box of relative width down to 1e-7 around the unconstrained minimiser (kind 4). The float oracle ends with
    (maxIterations, 2), the loop's `s == n` exit, the f64 oracle on the same rounded data with (solved, 0), and the problem
    fails the margin screen down to 1e-6; the device was measured at (solved, 1). A difference there is rounding, which the
    script tallies as such; this keeps the record that it is."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_boxqp.py")
    spec = importlib.util.spec_from_file_location("fuzz_boxqp", path)
    fuzz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fuzz)
    P, q, l, u = fuzz.case(44, np.float32)
    assert P.shape == (128, 128) and B.cond2(P) <= 40
    P64, q64, l64, u64 = (a.astype(np.float64) for a in (P, q, l, u))
    s32, _, i32 = oracle.solve_box_qp(P, q, l, u, dtype=np.float32)
    s64, x64, i64 = oracle.solve_box_qp(P64, q64, l64, u64)
    assert (s32, i32) == (STATUS_MAX_ITERATIONS, 2) and (s64, i64) == (0, 0)
    assert not B.margin_screened(P64, q64, l64, u64, x64, 1e-6)
    assert sorted({fuzz.case(s, np.float32)[0].shape[0] for s in range(120)})[-1] > 64          # float reaches the large classes
