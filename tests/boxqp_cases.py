"""Seeded families of small box-constrained QPs for the batched BOXCQP tests of both layouts (tests/test_batched_boxqp_host.py
and test_batched_boxqp16_host.py on the CPU, tests/test_gpu_batched_boxqp.py and test_gpu_batched_boxqp16.py on the device),
and what the tests share: the oracle's answers, the margin screen, the KKT check, and the device tests' comparison rules
(solve, same_bits, x_tolerance, check_against_oracle). Nothing here needs a device but a call of solve or solve_single.
The one-problem entry M.solveBoxQP (tests/test_boxqp_single_host.py, tests/test_gpu_boxqp_single.py) takes the same families at
its own orders, 16 problems each, with a margin of its own (NS_SINGLE, SINGLE_MARGIN below) and the constructions at the end.

A problem: P = A^T A / m + delta I (A m x n standard normal, m = n + 4, delta = 0.05; redrawn until cond_2(P) <= 1e3), q
standard normal scaled by 2, bounds l = c - w, u = c + w around a centre c ~ N(0, 1) of half-width w ~ U(0.05, 1.5), each
side infinite with probability 0.1: about half the variables end on a bound. The float tests solve the problem ROUNDED to
float (P, q, l, u cast to float32), and every reference computed in double takes those rounded numbers.

MARGIN SCREEN (exact status / iteration / active-set comparisons only): at the f64 oracle's solution x, with g = P x + q,
  * a variable on a bound (x_i == l_i or x_i == u_i) has its multiplier (g_i at a lower bound, -g_i at an upper one) at least
    1e-3 (1 + (|P| |x| + |q|)_i) -- the size of the terms the multiplier is the sum of -- above zero;
  * a free variable has both slacks x_i - l_i and u_i - x_i at least 1e-3 (1 + |bound|) above zero (an infinite bound passes).
A problem that fails the screen is one where a rounding error may legitimately change the path of the active-set loop. The
screened-out share of a family is capped at 10 % (asserted on the CPU from the oracle alone).
"""
import functools

import numpy as np

import mir_optim_amd as M

NS = (1, 2, 3, 5, 8)
NS16 = (9, 13, 16)                     # the 16-wide layout: lane 8 a row of its own, padding rows inside the row, none
FAMILY_COUNT = 64
COUNTS = (1, 3, 4, 5, 7, 257)
MAX_SCREENED_OUT = 0.10
DTYPES = (np.float32, np.float64)

# the one-problem entry (M.solveBoxQP; tests/test_boxqp_single_host.py, tests/test_gpu_boxqp_single.py): both sides of every
# edge between its kernel classes (n <= 16 / 32 / 64 / 128 in LDS, <= 256 with the factor in global memory, any n above),
# one short of a full 16-row block, and 16 problems an order. The 1e-3 margin leaves 2 of 16 problems at n = 256 (the
# chance that one of n variables lies within the margin of a flip grows with n): float gets ten times the largest distance
# its oracle shows from the f64 oracle on these families (3.4e-6), double a margin five orders above its distances.
NS_SINGLE = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
EDGE_NS = (2, 16, 17, 64, 65, 128, 129, 256, 257)
SINGLE_COUNT = 16
SINGLE_MARGIN = {np.float32: 3e-5, np.float64: 1e-8}
SINGLE_MAX_SCREENED_OUT = 2            # problems of SINGLE_COUNT


def cond2(P):
    w = np.linalg.eigvalsh(np.asarray(P, dtype=np.float64))
    return w[-1] / w[0]


def random_problem(rng, n, width=1.0):
    m = n + 4
    while True:
        A = rng.standard_normal((m, n))
        P = A.T @ A / m + 0.05 * np.eye(n)
        if cond2(P) <= 1e3:
            break
    q = 2.0 * rng.standard_normal(n)
    c = rng.standard_normal(n)
    w = width * rng.uniform(0.05, 1.5, n)
    l, u = c - w, c + w
    l[rng.random(n) < 0.1] = -np.inf
    u[rng.random(n) < 0.1] = np.inf
    return P, q, l, u


@functools.lru_cache(maxsize=None)
def family(n, dtype=np.float64, seed=20260, count=FAMILY_COUNT):
    """count problems of order n as float64 arrays holding values representable in `dtype`: P count x n x n (full symmetric),
    q, l, u count x n. The same (n, seed) gives the same problems; float32 rounds them."""
    rng = np.random.default_rng([seed, n])
    probs = [random_problem(rng, n) for _ in range(count)]
    out = [np.stack([p[k] for p in probs]) for k in range(4)]
    out = [a.astype(dtype).astype(np.float64) for a in out]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def qp_settings(oracle, dtype, relTolerance=None, absTolerance=None, maxIterations=None):
    s = oracle.default_settings(dtype).qpSettings
    if relTolerance is not None:
        s.relTolerance = relTolerance
    if absTolerance is not None:
        s.absTolerance = absTolerance
    if maxIterations is not None:
        s.maxIterations = maxIterations
    return s


def oracle_solve(oracle, P, q, l, u, dtype, settings=None, x0=None):
    """oracle.solve_box_qp over a batch: (status[count], x[count, n] as float64, iterations[count])."""
    count, n = q.shape
    st = np.zeros(count, dtype=np.int32); it = np.zeros(count, dtype=np.int32); x = np.zeros((count, n))
    shared = np.ndim(l) == 1
    for p in range(count):
        lp, up = (l, u) if shared else (l[p], u[p])
        if x0 is None:
            st[p], xp, it[p] = oracle.solve_box_qp(np.tril(P[p]), q[p], lp, up, settings=settings, dtype=dtype)
        else:
            st[p], xp, it[p] = oracle.solve_box_qp(np.tril(P[p]), q[p], lp, up, settings=settings, dtype=dtype, x0=x0[p],
                                                   unconstrained_solution=True)
        x[p] = xp
    return st, x, it


_ORACLE = {}


def oracle_family(oracle, n, dtype, data_dtype=None, count=FAMILY_COUNT):
    """The oracle's answers in `dtype` for family(n, data_dtype or dtype, count=count), computed once and shared (read-only)."""
    data_dtype = data_dtype or dtype
    key = (n, np.dtype(dtype).name, np.dtype(data_dtype).name, count)
    if key not in _ORACLE:
        res = oracle_solve(oracle, *family(n, data_dtype, count=count), dtype)
        for a in res:
            a.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def active_set(x, l, u):
    """-1 on the lower bound, 1 on the upper bound, 0 free: a bound variable is set to its bound exactly (QP:246, 253)."""
    x, l, u = np.broadcast_arrays(np.asarray(x, dtype=np.float64), l, u)
    return np.where(x == l, -1, np.where(x == u, 1, 0))


def margin_screened(P, q, l, u, x64, margin=1e-3):
    """True when the problem passes the margin screen at the f64 oracle's solution x64 (module docstring)."""
    g = P @ x64 + q
    scale = np.abs(P) @ np.abs(x64) + np.abs(q)
    fl = active_set(x64, l, u)
    for i in range(q.size):
        if fl[i] != 0:
            mult = g[i] if fl[i] < 0 else -g[i]
            if not mult >= margin * (1 + scale[i]):
                return False
        else:
            for slack, b in ((x64[i] - l[i], l[i]), (u[i] - x64[i], u[i])):
                if np.isfinite(b) and not slack >= margin * (1 + abs(b)):
                    return False
    return True


def screen_family(oracle, n, dtype, margin=1e-3, count=FAMILY_COUNT):
    """Boolean mask over family(n, dtype, count=count): the margin screen at the f64 oracle's solution of the same (rounded) data."""
    P, q, l, u = family(n, dtype, count=count)
    st, x64, _ = oracle_family(oracle, n, np.float64, dtype, count)
    return np.array([st[p] == 0 and margin_screened(P[p], q[p], l[p], u[p], x64[p], margin) for p in range(q.shape[0])])


def kkt_factor(P, q, l, u, x, eps):
    """The smallest factor f for which x passes the KKT check with tau_i = f eps (|P| |x| + |q|)_i, in numpy float64; inf when
    x leaves [l, u]. The tests assert f <= KKT_FACTOR."""
    x = np.asarray(x, dtype=np.float64)
    if not (np.all(l <= x) and np.all(x <= u)):
        return np.inf
    g = P @ x + q
    tau1 = eps * (np.abs(P) @ np.abs(x) + np.abs(q))
    fl = active_set(x, l, u)
    viol = np.where(fl < 0, -g, np.where(fl > 0, g, np.abs(g)))          # what must stay below tau
    viol = np.where((l == u), 0.0, viol)                                 # a fixed variable carries any multiplier
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(viol > 0, viol / tau1, 0.0)
    return float(np.max(f))


KKT_FACTOR = 8.0


def mixed_wave(oracle, n, dtype, seed=777, budget=4000):
    """Four problems of order n that need 0, 1, 2 and >= 3 active-set iterations by the oracle in `dtype` (status solved, margin
    screened), found by a fixed-seed search (every fourth draw has bounds eight times as wide: a feasible unconstrained
    minimiser is rare at n = 8 otherwise); classes that do not exist for this n are absent from the returned dict
    {class: (P, q, l, u)}. n = 1 has only 0 and 1: a one-variable problem whose minimiser lies outside [l, u] is moved to the
    violated bound in step 1, where the convex objective's slope has the multiplier's sign, so step 1 ends the loop."""
    rng = np.random.default_rng([seed, n])
    found = {}
    for trial in range(budget):
        P, q, l, u = [a.astype(dtype).astype(np.float64) for a in random_problem(rng, n, 8.0 if trial % 4 == 3 else 1.0)]
        st, x, it = oracle.solve_box_qp(np.tril(P), q, l, u, dtype=dtype)
        cls = min(int(it), 3)
        if st != 0 or cls in found:
            continue
        st64, x64, _ = oracle.solve_box_qp(np.tril(P), q, l, u)
        if st64 == 0 and margin_screened(P, q, l, u, x64):
            found[cls] = (P, q, l, u)
            if len(found) == (2 if n == 1 else 4):
                break
    return found


# ---------------------------------------------------------------- what the device tests of both layouts share
def solve(P, q, l, u, dtype, **kw):
    st, x, it = M.solveBoxQPBatched(P, q, l, u, dtype=dtype, **kw)
    assert x.dtype == dtype and st.shape == it.shape == (len(q),) and x.shape == q.shape
    return st, x, it


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return all(np.array_equal(bits(x) if x.dtype.kind == "f" else x, bits(y) if y.dtype.kind == "f" else y) for x, y in zip(a, b))


def x_tolerance(dtype, P, x64, xo):
    """per-problem bound on max|x - x64| (the device tests' module docstrings); xo: the same-precision oracle's x"""
    eps = np.finfo(dtype).eps
    if dtype == np.float64:
        return np.array([8 * eps * cond2(P[p]) * np.max(np.abs(x64[p])) for p in range(len(P))])
    shown = float(np.max(np.abs(xo - x64)))
    tol = max(4 * shown, 4 * eps * float(np.max(np.abs(x64))))
    print(f"float oracle's largest distance from the f64 oracle: {shown:.3e}; tolerance {tol:.3e}")
    return np.full(len(P), tol)


def check_against_oracle(dev, ora, ora64, data, dtype, screened, idx=None):
    """dev, ora, ora64: (status, x, iterations) of the device, the same-precision oracle and the f64 oracle on data = (P, q, l, u)
    (bounds per problem); idx: the problems of the oracle arrays the device solved, in order"""
    P, q, l, u = data
    idx = np.arange(len(q)) if idx is None else idx
    st, x, it = dev
    x = x.astype(np.float64)
    so, xo, io = (a[idx] for a in ora)
    s64, x64, _ = (a[idx] for a in ora64)
    P, q, l, u, scr = P[idx], q[idx], l[idx], u[idx], screened[idx]
    assert np.array_equal(st, so), (st, so)
    assert np.array_equal(it[scr], io[scr]), (it[scr], io[scr])
    assert np.array_equal(active_set(x, l, u)[scr], active_set(xo, l, u)[scr])
    eps = np.finfo(dtype).eps
    ok = st == 0
    need = [kkt_factor(P[p], q[p], l[p], u[p], x[p], eps) for p in np.flatnonzero(ok)]
    print(f"KKT factor needed by the device's x: {max(need, default=0):.2f} (allowed {KKT_FACTOR})")
    assert all(f <= KKT_FACTOR for f in need), max(need)
    both = ok & (s64 == 0)
    tol = x_tolerance(dtype, P, x64, xo)
    dist = np.max(np.abs(x - x64), axis=1)
    print(f"largest distance from the f64 oracle: {np.max(dist[both], initial=0):.3e}")
    assert np.all(dist[both] <= tol[both]), (dist[both] / tol[both]).max()


# ---------------------------------------------------------------- the one-problem entry (M.solveBoxQP)
def kernel_class(n):
    """which kernel of mir_solve_box_qp_gpu_* an order runs (csrc/solve_types.h: solve_nb; the same in both precisions)"""
    return ("k_box_qp<NB=1>" if n <= 16 else "k_box_qp<NB=2>" if n <= 32 else "k_box_qp<NB=4>" if n <= 64 else
            "k_box_qp<NB=8>" if n <= 128 else "k_box_qp<NB=0>" if n <= 256 else "k_box_qp_big")


def lower_only(P):
    """the lower triangle with NaN above the diagonal: only the lower triangle may be read (QP:109)"""
    return np.tril(P) + np.triu(np.full(P.shape, np.nan), 1)


def solve_single(P, q, l, u, dtype, **kw):
    """M.solveBoxQP over a batch (l, u shared or per problem; x per problem), one launch a problem: (status[count],
    x[count, n] in dtype, iterations[count]), the shapes check_against_oracle takes."""
    count, n = q.shape
    st = np.zeros(count, dtype=np.int32); it = np.zeros(count, dtype=np.int32); x = np.zeros((count, n), dtype=dtype)
    shared = np.ndim(l) == 1
    x0 = kw.pop("x", None)
    for p in range(count):
        lp, up = (l, u) if shared else (l[p], u[p])
        s, xp, it[p] = M.solveBoxQP(lower_only(P[p]), q[p], lp, up, x=None if x0 is None else x0[p], dtype=dtype, **kw)
        assert xp.dtype == dtype and xp.shape == (n,)
        st[p], x[p] = int(s), xp
    return st, x, it


def refined_solve(A, b):
    """float64 solve polished with residuals accumulated in long double (refined_solve of tests/test_gpu_kernels.py)"""
    x = np.linalg.solve(A, b).astype(np.longdouble)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(4):
        r = np.asarray(bl - Al @ x, dtype=np.float64)
        x = x + np.linalg.solve(A, r)
    return np.asarray(x, dtype=np.float64)


def solution_on_active_set(P, q, l, u, x):
    """The extended-precision minimiser with x's bound variables held at their bounds: P_FF x_F = -(q_F + P_FB x_B)."""
    fl = active_set(x, l, u)
    F = fl == 0
    xs = np.where(fl < 0, l, np.where(fl > 0, u, 0.0))
    if F.any():
        Pl = P.astype(np.longdouble)
        rhs = -(q.astype(np.longdouble)[F] + Pl[np.ix_(F, ~F)] @ xs.astype(np.longdouble)[~F])
        xs[F] = refined_solve(P[np.ix_(F, F)], np.asarray(rhs, dtype=np.float64))
    return xs


@functools.lru_cache(maxsize=None)
def all_active_family(n, dtype, count=SINGLE_COUNT, seed=20260):
    """Every bound active, at any order: P' = (P + 3 diag(P)) / 4 of the family's P (a convex combination of SPD matrices,
    cond_2 no worse than the family's up to the diagonal's spread), d ~ U(0.5, 2) drawn again until P' d > 0.05 in every
    component, z ~ N(0, 1), q = P' d - P' z, l = z, u = z + 1: the unconstrained minimiser z - d lies below l everywhere, step
    1 puts every variable on its lower bound (s == 0: no reduced system), the multipliers are P' d > 0: status 0, 1 iteration,
    x == l. Returns (P', q, l, u, draws of d)."""
    rng = np.random.default_rng([seed, n, 1])
    P = family(n, dtype, count=count)[0]
    Ps, qs, ls, draws = [], [], [], 0
    for p in range(count):
        Pp = ((P[p] + 3 * np.diag(np.diag(P[p]))) / 4).astype(dtype).astype(np.float64)
        while True:
            d = rng.uniform(0.5, 2.0, n); draws += 1
            if np.all(Pp @ d > 0.05):
                break
        z = rng.standard_normal(n)
        Ps.append(Pp); qs.append((Pp @ d - Pp @ z).astype(dtype).astype(np.float64)); ls.append(z.astype(dtype).astype(np.float64))
    P, q, l = np.stack(Ps), np.stack(qs), np.stack(ls)
    u = (l + 1).astype(dtype).astype(np.float64)
    for a in (P, q, l, u):
        a.setflags(write=False)
    return P, q, l, u, draws


def indefinite_positions(n):
    """pivots to spoil: the first, the last of the first 16-row block, the first of the second, the middle, the last two"""
    return sorted({int(np.clip(k, 0, n - 1)) for k in (0, 15, 16, n // 2, n - 2, n - 1)})


def indefinite(P, k):
    Pb = P.copy()
    Pb[k, k] = -1.0
    return Pb


@functools.lru_cache(maxsize=None)
def badly_scaled_family(n, count=SINGLE_COUNT, seed=20260):
    """float32 only: D P D of the family's P with D = 10^U(-1.5, 1.5) (the float scaling of scripts/fuzz_boxqp.py), rounded to
    float32, and the family's q: ?poequ / ?laqsy must equilibrate. Returns (P, q) as float64 arrays of float32 values."""
    rng = np.random.default_rng([seed, n, 2])
    P, q, _, _ = family(n, np.float32, count=count)
    d = 10.0 ** rng.uniform(-1.5, 1.5, (count, n))
    Ps = (P * d[:, :, None] * d[:, None, :]).astype(np.float32).astype(np.float64)
    Ps.setflags(write=False)
    return Ps, q


def worst_figures(dev, ora, ora64, data, dtype):
    """(largest KKT factor the device's solved x need, largest max|x - x64| / x_tolerance): what check_against_oracle asserts
    on, as two numbers to print"""
    P, q, l, u = data
    st, x, _ = dev
    x = x.astype(np.float64)
    ok = st == 0
    kkt = max((kkt_factor(P[p], q[p], l[p], u[p], x[p], np.finfo(dtype).eps) for p in np.flatnonzero(ok)), default=0.0)
    both = ok & (ora64[0] == 0)
    tol = x_tolerance(dtype, P, ora64[1], ora[1])
    ratio = float(np.max((np.max(np.abs(x - ora64[1]), axis=1) / tol)[both], initial=0.0))
    return kkt, ratio


# l == u beyond the batched orders: BOXCQP is not guaranteed to end, and from n = 16 on the reference's loop cycles on most
# of these problems until its default limit of 10 n + 100 steps (every problem from n = 64 on; tests/test_boxqp_single_host.py),
# which takes the oracle alone several seconds a case at n = 256. The problems that end do so within 5 steps, so the tests of
# the one-problem entry set this limit on both sides: the same answers on the problems that end, maxIterations on the others.
EQUAL_BOUNDS_MAX_ITERATIONS = 64


def equal_bounds_centre(l, u, dtype):
    """where test_equal_bounds fixes a variable: the middle of a finite box, 0.25 otherwise, rounded to dtype"""
    return np.where(np.isfinite(l) & np.isfinite(u), (np.nan_to_num(l) + np.nan_to_num(u)) / 2, 0.25).astype(dtype).astype(np.float64)
