"""Kernel-level cases of the read-only Broyden sweep (csrc/broyden_lr.h: k_broyden_lr, k_lr_reduce, k_lr_finish, k_lr_sumsq,
k_lr_sumsq_final, k_lr_flush) over the unit entries mir_lsq_lr_pass_* / mir_lsq_lr_flush_*: the cells, the generators, the
references with their derived bounds, a numpy restatement of a pass in the kernels' type (the stand-in the CPU tier plants
mistakes in) and the named assertions shared by tests/test_lr_cell_coverage.py (CPU) and tests/test_gpu_lr_cells.py (device).
Nothing here needs a device but run_pass / run_flush. Guard bands, gamma, the bit comparison and the exact step come from
tests/jtj_cases.py, `named` and `tsum` from tests/lm_solve_cases.py.

A PASS with k pending terms (J_{k-1} = J0 + sum_{l<k} U_l D_l^T, U_l = U[l], D_l = D[l]; nd = -(1 / dx_dot)):
    coef_l = D_l.dx                                   s_i = J0_i.dx + sum_l U_l[i] coef_l
    u_i    = nd ((y_old_i - y_i) + s_i)               -> U[k]
    v0 = J0^T u, g0 = J0^T y, w_l = U_l.u, h_l = U_l.y (0 for l >= k), uu = u.u, uy = u.y, yy = y.y   -> the reduced vector
    v  = v0 + sum_l D_l w_l                            Jy = g0 + sum_l D_l h_l + dx uy,  jy_inf = max |Jy|,  D[k] = dx
    JJ_ij += uu dx_i dx_j + (v_i dx_j + dx_i v_j)
A FLUSH: J_i += U_0[i] D_0 + ... + U_{k-1}[i] D_{k-1}, in that order.

CELLS (every one in f32 and f64; `off` = 1 shifts J one element off the 16-byte grid, which takes an even n to the non-vector
instance). kind "pass": mode "plain" (sweep, reduce, finish), "go*" (speculative sweep on a record that lets a pass follow:
no finish) or one of NOGO (a record that does not: ||y||^2 and zeros). kind "flush". kind "chain": passes k = 0 .. 3 through the
entry, then a flush.

CHECKS, each raising AssertionError("<name>: ...") through lm_solve_cases.named:
  exact      small-integer data: U[k], the reduced vector, JJ, Jy, the flushed J equal the formulas above bit for bit (sign of
             zero open): every value is a multiple of 1/16 and every sum of absolute values stays below 2^24 / 16 (asserted by
             the generator), so every partial sum in any order is exact in f32 and f64
  u          U[k] within E_i of the wide u_i (derivation at check_u)
  reduced    v0, g0, w, h, uu, uy, yy within gamma_m |a|.|b| of wide sums formed from the DOWNLOADED U[k]
  JJ, Jy     from the downloaded reduced vector, first-order bounds over k + 2 terms resp. the three products (check_finish)
  symmetry   JJ_out bitwise symmetric
  bits       reduced[lr_yy] == sums[0]; jy_inf == max |Jy|; D[k] == dx; a second call gives the same bits
  nogo       every partial entry but lr_yy is +0, lr_yy as above
  flush      the flushed J within gamma_{2k} (|J0| + |U|^T|D|) of J0 + U^T D
  chain      JJ, Jy of four chained passes against J_4^T J_4, J_4^T y under jtj_cases.product_bound
What did not move (guard bands, read-only inputs, the other columns of U and rows of D, the state, the record) is asserted by
run_pass / run_flush themselves."""
import collections

import numpy as np

from mir_optim_amd import api
import jtj_cases as JC
from jtj_cases import Guarded, gamma, same_bits, bits, UNIT, REF_UNIT, UINT
from lm_solve_cases import named, tsum

DTYPES = (np.float32, np.float64)
NS = (1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258, 511, 512)
M_N = 133                    # the n axis: two workgroups, m % 4 == 1, 5 groups a wave (no multiple of the unroll 4 or 2)
SMALL_MS = (1, 3, 4, 5, 127, 128, 129)
M_RAGGED = 769               # 7 workgroups, 7 groups a wave, the last wave 4
M_REDUCE = 4 * 32 * 33 + 1   # 34 partials: 17 of the 32 reduction ranges take 2, 15 none
M_GRID = 131077              # lr_blocks at its upper limit of 1024 on a device of 256 compute units
SWEEP_KS = (0, 1, 4, 5, 15)
FLUSH_KS = (1, 2, 15, 16)
CHAIN_NS = (20, 50, 100)     # one shape per class with n <= 128
CHAIN_PASSES = 4
NOGO = ("qp_status", "dx_nan", "x_nan", "step_too_long", "grad_small", "null_step", "abs_tol", "rel_tol")
GO = ("go", "go_other_flags")
COUNT_MAX = api.LM_SOLVE_CHAIN

Cell = collections.namedtuple("Cell", "kind dtype m n k off mode count")


def _cells():
    c = []
    for dt in DTYPES:
        for n in NS:                                     # every class: odd n, even n aligned and shifted, full width, first n above
            for off in ((0, 1) if n % 2 == 0 else (0,)):
                c += [Cell("pass", dt, M_N, n, 5, off, "plain", 1), Cell("flush", dt, M_N, n, 2, off, "", 0)]
        for m in SMALL_MS + (M_RAGGED,):
            c += [Cell("pass", dt, m, 7, 4, 0, "plain", 1), Cell("pass", dt, m, 40, 4, 0, "plain", 1)]
            c += [Cell("flush", dt, m, 7, 4, 0, "", 0), Cell("flush", dt, m, 40, 4, 0, "", 0)]
        c += [Cell("pass", dt, M_REDUCE, 5, 1, 0, "plain", COUNT_MAX), Cell("pass", dt, M_REDUCE, 512, 1, 0, "plain", 1),
              Cell("pass", dt, M_REDUCE, 5, 1, 0, "qp_status", COUNT_MAX), Cell("flush", dt, M_REDUCE, 512, 1, 0, "", 0)]
        c += [Cell("pass", dt, M_GRID, 3, 1, 0, "plain", 1), Cell("pass", dt, M_GRID, 8, 1, 0, "go", COUNT_MAX),
              Cell("flush", dt, M_GRID, 3, 1, 0, "", 0)]
        for k in SWEEP_KS:
            c += [Cell("pass", dt, M_N, 35, k, 0, "plain", 1), Cell("pass", dt, M_N, 36, k, 0, "plain", 1)]
        for k in FLUSH_KS:
            c += [Cell("flush", dt, M_N, 35, k, 0, "", 0), Cell("flush", dt, M_N, 36, k, 0, "", 0)]
        c += [Cell("flush", dt, M_N, 512, 16, 0, "", 0)]                 # 64 KiB of dynamic LDS in f64
        for mode in GO + NOGO:
            c += [Cell("pass", dt, M_N, 36, 4, 0, mode, COUNT_MAX if mode in ("go", "rel_tol") else 1)]
        c += [Cell("pass", dt, M_N, 35, 4, 0, "go", 1), Cell("pass", dt, M_N, 35, 4, 0, "null_step", 1)]
        c += [Cell("chain", dt, M_N, n, 0, 0, "", 0) for n in CHAIN_NS]
    assert len(set(c)) == len(c)
    return tuple(c)


CELLS = _cells()


def cell_id(c):
    return (f"{np.dtype(c.dtype).name}-{c.kind}-m{c.m}-n{c.n}-k{c.k}" + ("-offset" if c.off else "") + (f"-{c.mode}" if c.mode else "")
            + (f"-count{c.count}" if c.count > 1 else ""))


def cell_classes(c):
    """the kernel instances a cell runs, through the library's own class function: {(element size, kernel, NCP, VEC)}"""
    es = np.dtype(c.dtype).itemsize
    cls = api.lr_class(es, c.n, aligned=(c.off == 0))
    return {(es, kern) + cls for kern in {"pass": ("sweep",), "flush": ("flush",), "chain": ("sweep", "flush")}[c.kind]}


# every instance launch_broyden.hip compiles of k_broyden_lr and k_lr_flush, written out by hand
LISTED = {(es, kern, ncp, vec) for es in (4, 8) for kern in ("sweep", "flush") for ncp in (1, 2, 4, 8, 16) for vec in (False, True)}


def blocks_by_hand(m, num_cu):
    """lr_blocks restated: a workgroup per 32 four-row groups, at most four a compute unit and 1024"""
    G = (m + 3) // 4
    return max(1, min((G + 31) // 32, 4 * num_cu, 1024))


def groups_per_wave(m, nblk):
    return -(-((m + 3) // 4) // (4 * nblk))


# ---------------------------------------------------------------- records of the speculative sweep
def spec_of(mode, dtype):
    """(record fields, absTolerance, relTolerance) of a speculative cell, values of the type. The go records sit ON the edge of
    both tolerance tests -- sqrt(new_dx_dot) = 1 one spacing above absTolerance, trial_xnorm one spacing above
    sqrt(new_dx_dot) relTolerance = 1/2 -- and "abs_tol" / "rel_tol" at equality, where lr_spec_go's `>` says no"""
    T = np.dtype(dtype).type
    rec = {"qp_status": 0, "flags": 0, "new_dx_dot": T(1), "trial_xnorm": np.nextafter(T(0.5), T(1)), "lambda": T(0.125),
           "predicted": T(-1), "qp_iterations": 3}
    at, rt = np.nextafter(T(1), T(0)), T(0.5)
    if mode == "go_other_flags":
        rec["flags"] = 8 | 64                            # trial not finite, helpers rescued: neither is in lr_spec_go's mask
    elif mode == "qp_status":
        rec["qp_status"] = 1
    elif mode in ("dx_nan", "x_nan", "step_too_long", "grad_small", "null_step"):
        rec["flags"] = {"dx_nan": api.LM_FLAG_DX_NAN, "x_nan": api.LM_FLAG_X_NAN, "step_too_long": api.LM_FLAG_STEP_TOO_LONG,
                        "grad_small": api.LM_FLAG_GRAD_SMALL, "null_step": api.LM_FLAG_NULL_STEP}[mode]
    elif mode == "abs_tol":
        at = T(1)
    elif mode == "rel_tol":
        rec["trial_xnorm"] = T(0.5)
    else:
        assert mode == "go"
    return rec, at, rt


def spec_go_by_hand(rec, at, rt):
    T = type(rec["new_dx_dot"])
    dxn = np.sqrt(rec["new_dx_dot"])
    return bool(rec["qp_status"] == 0 and not (rec["flags"] & (1 | 2 | 4 | 32 | 16)) and dxn > T(at) and rec["trial_xnorm"] > dxn * T(rt))


# ---------------------------------------------------------------- generators
def _wide(dtype):
    return np.longdouble if np.dtype(dtype) == np.float64 else np.float64


EXACT_LIMIT = 2.0 ** 24 / 16


def exact_inputs(m, n, k, dtype, count=1):
    """integers: J in [-3, 3] with jtj_cases' asymmetric column, U, D in [-1, 1], y, y_old in [-3, 3] ([-1, 1] for the three of them
    above 2^14 rows, where sums of 3 x 3 products would leave the bound), JJ symmetric in [-8, 8];
    dx = 2 jtj_cases.exact_dx(n): entries 0, +-1 (-2 for n = 1), dx.dx = 4 or 2. Then u is a multiple of 1/4, every product of
    two values a multiple of 1/16, and assert_exact says that every sum the kernels form stays below EXACT_LIMIT = 2^20 in
    absolute values: exact in f32 (24 bits) and f64 whatever the order"""
    rng = JC._seed(11, m, n, k)
    amp = 3 if m <= 1 << 14 else 1
    J = rng.integers(-amp, amp + 1, size=(m, n)).astype(dtype)
    J[:, JC.asym_col(n)] = (np.arange(m) % (2 * amp - 1) - (amp - 1)).astype(dtype)
    U = rng.integers(-1, 2, size=(k, m)).astype(dtype)
    D = rng.integers(-1, 2, size=(k, n)).astype(dtype)
    y = rng.integers(-amp, amp + 1, size=(count, m)).astype(dtype)
    y_old = rng.integers(-amp, amp + 1, size=m).astype(dtype)
    A = rng.integers(-4, 5, size=(n, n))
    JJ = (A + A.T).astype(dtype)
    dx = (2 * JC.exact_dx(n)).astype(dtype)
    inp = dict(J=J, U=U, D=D, y=y, y_old=y_old, JJ=JJ, dx=dx, dx_dot=np.array([dx.astype(np.float64) @ dx], dtype=dtype))
    assert inp["dx_dot"][0] in (2.0, 4.0) and set(np.unique(dx)) <= {-2.0, -1.0, 0.0, 1.0}
    return inp


def assert_exact(inp, ref):
    """the magnitude bound of exact_inputs on the wide evaluation `ref` of the same inputs"""
    a = np.abs
    J, U, y, u = a(inp["J"].astype(np.float64)), a(inp["U"].astype(np.float64)), a(inp["y"][0].astype(np.float64)), a(ref["u"].astype(np.float64))
    sums = [J.T @ u, J.T @ y, U @ u, U @ y, u @ u, u @ y, y @ y, a(ref["s_abs"]), a(inp["JJ"]) + a(ref["term_abs"]), a(ref["Jy_abs"]), a(ref["v_abs"])]
    top = max(float(np.max(v)) for v in sums if np.size(v))
    assert top < EXACT_LIMIT, top
    for key in ("u", "reduced", "JJ", "Jy"):
        v = np.asarray(ref[key], dtype=np.float64)
        assert np.array_equal(16 * v, np.rint(16 * v)), key
    return top


def random_inputs(m, n, k, dtype, count=1, seed=0):
    """jtj_cases.random_case's scales: J, U ~ N(0, 1) (J with the asymmetric column), y near y_old, steps of 0.05 N(0, 1). JJ is
    any symmetric matrix (a pass only adds to it; `chain` starts from fl(J0^T J0)); dx_dot = fl(dx.dx)"""
    rng = JC._seed(12, m, n, k, seed)
    J = rng.standard_normal((m, n)).astype(dtype)
    J[:, JC.asym_col(n)] = (np.arange(m) % 5 - 2).astype(dtype)
    U = rng.standard_normal((k, m)).astype(dtype)
    D = (0.05 * rng.standard_normal((k, n))).astype(dtype)
    y_old = rng.standard_normal(m).astype(dtype)
    y = (y_old[None, :] + 0.1 * rng.standard_normal((count, m))).astype(dtype)
    A = rng.standard_normal((n, n))
    JJ = (A + A.T).astype(dtype)
    dx = (0.05 * rng.standard_normal(n)).astype(dtype)
    W = _wide(dtype)
    return dict(J=J, U=U, D=D, y=y, y_old=y_old, JJ=JJ, dx=dx, dx_dot=np.array([dx.astype(W) @ dx.astype(W)]).astype(dtype))


# ---------------------------------------------------------------- the formulas in the wide type
def wide_pass(inp, W=None):
    """the header's formulas on the inputs as given, in W (default: longdouble for f64 inputs, float64 for f32). Also the sums of
    absolute values that the bounds and assert_exact need"""
    dt = inp["J"].dtype
    W = W or _wide(dt)
    J, U, D, y, yo, JJ, dx = (inp[key].astype(W) for key in ("J", "U", "D", "y", "y_old", "JJ", "dx"))
    y = y[0]
    k, n = U.shape[0], J.shape[1]
    nd = -(1 / W(inp["dx_dot"][0]))
    coef = D @ dx
    s = J @ dx + U.T @ coef
    u = nd * ((yo - y) + s)
    red = np.zeros(api.lr_len(n), dtype=W)
    red[:n], red[n:2 * n] = J.T @ u, J.T @ y
    red[2 * n:2 * n + k], red[2 * n + api.LR_MAX:2 * n + api.LR_MAX + k] = U @ u, U @ y
    red[-3:] = u @ u, u @ y, y @ y
    out = dict(u=u, reduced=red, coef=coef, nd=nd)
    out["s_abs"] = np.abs(J) @ np.abs(dx) + np.abs(U).T @ (np.abs(D) @ np.abs(dx))
    out.update(wide_finish(red, inp, W))
    return out


def wide_finish(red, inp, W=None):
    """v, Jy and the JJ term from a reduced vector (the wide one, or a downloaded one), in W"""
    dt = inp["J"].dtype
    W = W or _wide(dt)
    D, JJ, dx = (inp[key].astype(W) for key in ("D", "JJ", "dx"))
    red = np.asarray(red).astype(W)
    k, n = D.shape[0], dx.size
    w, h = red[2 * n:2 * n + k], red[2 * n + api.LR_MAX:2 * n + api.LR_MAX + k]
    uu, uy = red[-3], red[-2]
    v = red[:n] + D.T @ w
    Jy = red[n:2 * n] + D.T @ h + dx * uy
    term = uu * np.outer(dx, dx) + (np.outer(v, dx) + np.outer(dx, v))
    a = np.abs
    return dict(v=v, Jy=Jy, term=term, JJ=JJ + term,
                v_abs=a(red[:n]) + a(D).T @ a(w), Jy_abs=a(red[n:2 * n]) + a(D).T @ a(h) + a(dx) * a(uy),
                term_abs=a(uu) * np.outer(a(dx), a(dx)) + np.outer(a(v), a(dx)) + np.outer(a(dx), a(v)))


def wide_flush(inp):
    W = _wide(inp["J"].dtype)
    J, U, D = (inp[key].astype(W) for key in ("J", "U", "D"))
    return J + U.T @ D, np.abs(J) + np.abs(U).T @ np.abs(D)


# ---------------------------------------------------------------- the stand-in: a pass restated in the kernels' type
MUTATIONS = ("drop_last_rows", "spare_row_twice", "skip_pending", "coef_next_D", "swap_y", "no_uu", "no_transpose_partner",
             "drop_last_col", "h_for_w")


def standin_pass(inp, order=0, mutate=None):
    """what run_pass returns for a plain pass, from numpy in the inputs' type; sums in one of tsum's three orders, no FMA"""
    dt = inp["J"].dtype
    T = dt.type
    J, U, D, Y, yo, JJ, dx = (inp[key] for key in ("J", "U", "D", "y", "y_old", "JJ", "dx"))
    y = Y[0]
    m, n = J.shape
    k = U.shape[0]
    Dc = np.roll(D, -1, axis=0) if mutate == "coef_next_D" else D
    coef = tsum(Dc * dx[None, :], order) if k else np.zeros(0, dtype=dt)
    Js, Us = J * dx[None, :], U.T * coef[None, :]
    if mutate == "skip_pending" and k:
        Us = Us[:, :-1]
    s = tsum(np.concatenate([Js, Us], axis=1), order)
    nd = -(T(1) / inp["dx_dot"][0])
    u = nd * ((y - yo) + s) if mutate == "swap_y" else nd * ((yo - y) + s)
    rows = np.arange(m)
    if mutate == "drop_last_rows":
        rows = rows[:m - m % 4]
    if mutate == "spare_row_twice":
        rows = np.append(rows, m - 1)
    Jr, Ur, ur, yr = J[rows], U[:, rows], u[rows], y[rows]
    if mutate == "drop_last_col" and n % 2:
        Jr = Jr.copy()
        Jr[:, -1] = 0
    red = np.zeros(api.lr_len(n), dtype=dt)
    red[:n], red[n:2 * n] = tsum((Jr * ur[:, None]).T, order), tsum((Jr * yr[:, None]).T, order)
    if k:
        red[2 * n:2 * n + k], red[2 * n + api.LR_MAX:2 * n + api.LR_MAX + k] = tsum(Ur * ur[None, :], order), tsum(Ur * yr[None, :], order)
    red[-3], red[-2], red[-1] = tsum(ur * ur, order), tsum(ur * yr, order), tsum(yr * yr, order)
    w, h = red[2 * n:2 * n + k], red[2 * n + api.LR_MAX:2 * n + api.LR_MAX + k]
    uu, uy = red[-3], red[-2]
    v, g = red[:n].copy(), red[n:2 * n].copy()
    for l in range(k):
        v = v + D[l] * w[l]
        g = g + D[l] * (w[l] if mutate == "h_for_w" else h[l])
    Jy = g + dx * uy
    i, j = np.indices((n, n))
    r, c = np.maximum(i, j), np.minimum(i, j)
    if mutate == "no_transpose_partner":
        term = (uu * dx[i]) * dx[j] + v[i] * dx[j]
    else:
        term = (T(0) if mutate == "no_uu" else (uu * dx[r]) * dx[c]) + (v[r] * dx[c] + dx[r] * v[c])
    Dout = np.concatenate([D, dx[None, :]])
    sums = np.array([red[-1]] + [tsum(yv * yv, order) for yv in Y[1:]], dtype=dt)      # (vector 0: the sweep's own walk over y)
    return dict(U_col=u.astype(dt), D=Dout, JJ=(JJ + term).astype(dt), Jy=Jy.astype(dt), reduced=red, partials=red[None, :].copy(),
                sums=sums, jy_inf=np.abs(Jy).max(), nblk=1)


# ---------------------------------------------------------------- the named assertions
def _g(k, dtype):
    """gamma_k of the kernels' type plus gamma_k of the reference's"""
    es = np.dtype(dtype).itemsize
    return gamma(k, UNIT[es]) + gamma(k, REF_UNIT[es])


def check_exact_pass(res, inp, finished=True):
    ref = wide_pass(inp)
    assert_exact(inp, ref)
    dt = inp["J"].dtype
    named("exact", same_bits(res["U_col"], ref["u"].astype(dt)), "U[k] at rows", np.flatnonzero(res["U_col"] != ref["u"].astype(dt))[:6])
    named("exact", same_bits(res["reduced"], ref["reduced"].astype(dt)), "reduced vector at", np.flatnonzero(res["reduced"] != ref["reduced"].astype(dt))[:6])
    if finished:
        named("exact", same_bits(res["JJ"], ref["JJ"].astype(dt)), "JJ at", np.argwhere(res["JJ"] != ref["JJ"].astype(dt))[:4].tolist())
        named("exact", same_bits(res["Jy"], ref["Jy"].astype(dt)), "Jy at", np.flatnonzero(res["Jy"] != ref["Jy"].astype(dt))[:6])


def check_u(res, inp):
    """U[k] against u_i = nd ((y_old_i - y_i) + s_i), nd = -(1 / dx_dot) on the dx_dot GIVEN (an input of the sweep).
    Rounding model (unit roundoff u, every operation rounded once or, contracted, not at all; sums in any order):
      coef_l = fl(D_l.dx): relative error gamma_n on sum_j |D_lj| |dx_j|;
      s_i: n + k products, n + k - 1 additions: gamma_{n+k} on |J0_i|.|dx|, gamma_{2n+k} on sum_l |U_l[i]| |D_l|.|dx| (coef's on top);
      t_i = fl(fl(y_old_i - y_i) + s_i): two more roundings: gamma_{n+k+2} (|y_old_i| + |y_i| + |J0_i|.|dx|) + gamma_{2n+k+2} (pending part);
      u_i = fl(fl(-1 / dx_dot) t_i): the division and the product: E_i = |nd| (the above) + gamma_2 |u_i|  (first order).
    The wide reference rounds the same operations in its own type: _g adds its gamma. Twice that, for every second-order term
    (all gammas are below 1e-2). Returns the largest error / bound."""
    dt = inp["J"].dtype
    W = _wide(dt)
    ref = wide_pass(inp)
    n, k = inp["dx"].size, inp["U"].shape[0]
    a = np.abs
    J, U, D, y, yo, dx = (a(inp[key].astype(W)) for key in ("J", "U", "D", "y", "y_old", "dx"))
    pend = U.T @ (D @ dx) if k else 0
    E = a(ref["nd"]) * (_g(n + k + 2, dt) * (yo + y[0] + J @ dx) + _g(2 * n + k + 2, dt) * pend) + _g(2, dt) * a(ref["u"])
    err = a(res["U_col"].astype(W) - ref["u"])
    named("u", np.all(err <= 2 * E), "worst error / bound", float(np.max(err / np.maximum(2 * E, np.finfo(np.float64).tiny))), "at row", int(np.argmax(err - 2 * E)))
    return float(np.max(err / np.maximum(2 * E, np.finfo(np.float64).tiny)))


def check_reduced(res, inp):
    """every entry of the reduced vector against a wide sum formed from the DOWNLOADED U[k] (exact in the wide type): an inner
    product of m terms in any order, contracted or not, is within gamma_m |a|.|b| (jtj_cases.product_bound); the reference's own
    gamma_m is added, and the float64 sum of the absolute values may be low by 1 + gamma_{m+1}(2^-53). Rows past m and columns
    l >= k add exact zeros. Returns the largest error / bound."""
    dt = inp["J"].dtype
    W = _wide(dt)
    J, U, y = (inp[key].astype(W) for key in ("J", "U", "y"))
    y = y[0]
    u = res["U_col"].astype(W)
    m, n = J.shape
    k = U.shape[0]
    L = api.LR_MAX
    ref, ab = np.zeros(api.lr_len(n), dtype=W), np.zeros(api.lr_len(n), dtype=W)
    a = np.abs
    ref[:n], ab[:n] = J.T @ u, a(J).T @ a(u)
    ref[n:2 * n], ab[n:2 * n] = J.T @ y, a(J).T @ a(y)
    ref[2 * n:2 * n + k], ab[2 * n:2 * n + k] = U @ u, a(U) @ a(u)
    ref[2 * n + L:2 * n + L + k], ab[2 * n + L:2 * n + L + k] = U @ y, a(U) @ a(y)
    ref[-3:], ab[-3:] = (u @ u, u @ y, y @ y), (u @ u, a(u) @ a(y), y @ y)
    bound = _g(m, dt) * (1 + gamma(m + 1, 2.0 ** -53)) * ab
    err = a(res["reduced"].astype(W) - ref)
    named("reduced", np.all(err <= bound), "entries", np.flatnonzero(err > bound)[:6], "of", api.lr_len(n), "worst error / bound",
          float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0)
    unused = np.r_[2 * n + k:2 * n + L, 2 * n + L + k:2 * n + 2 * L]
    named("reduced", np.all(bits(res["reduced"][unused]) == 0), "w / h beyond the pending columns are not +0")
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def check_finish(res, inp):
    """JJ, Jy from the DOWNLOADED reduced vector r (exact in the wide type), n^2 work.
      v_j  = r_j + sum_l D_lj w_l: k products and k additions, each value through at most k + 1 roundings (k contracted):
             |dv_j| <= gamma_{k+2} (|r_j| + sum_l |D_lj| |w_l|) =: Ev_j       (k + 2: the issue's count, one above what is needed)
      Jy_j = r_{n+j} + sum_l D_lj h_l + dx_j uy: k + 1 products, k + 1 additions: gamma_{k+2} (|r_{n+j}| + sum_l |D_lj| |h_l| + |dx_j| |uy|)
      term_ij = (uu dx_r) dx_c + (v_r dx_c + dx_r v_c): each of the three products passes at most 3 roundings (its own one or
             two and the additions behind it): gamma_3 (|uu| |dx_i| |dx_j| + |v_i| |dx_j| + |dx_i| |v_j|) + |dx_j| Ev_i + |dx_i| Ev_j
      JJ_out = fl(JJ_in + term): u |JJ_in + term| more.
    First order; twice that for the second-order terms. Returns the largest error / bound of (JJ, Jy)."""
    dt = inp["J"].dtype
    W = _wide(dt)
    es = dt.itemsize
    k = inp["U"].shape[0]
    f = wide_finish(res["reduced"], inp)
    a = np.abs
    dx = a(inp["dx"].astype(W))
    Ev = _g(k + 2, dt) * f["v_abs"]
    bJy = 2 * _g(k + 2, dt) * f["Jy_abs"]
    bJJ = 2 * (_g(3, dt) * f["term_abs"] + np.outer(Ev, dx) + np.outer(dx, Ev) + (UNIT[es] + REF_UNIT[es]) * a(f["JJ"]))
    eJy, eJJ = a(res["Jy"].astype(W) - f["Jy"]), a(res["JJ"].astype(W) - f["JJ"])
    tiny = np.finfo(np.float64).tiny
    named("Jy", np.all(eJy <= bJy), "worst error / bound", float(np.max(eJy / np.maximum(bJy, tiny))), "at", int(np.argmax(eJy - bJy)))
    named("JJ", np.all(eJJ <= bJJ), "worst error / bound", float(np.max(eJJ / np.maximum(bJJ, tiny))), "at",
          np.unravel_index(int(np.argmax(eJJ - bJJ)), eJJ.shape))
    return float(np.max(eJJ / np.maximum(bJJ, tiny))), float(np.max(eJy / np.maximum(bJy, tiny)))


def check_bits(res, inp, finished=True):
    """the identities held to the bit on any data"""
    dt = inp["J"].dtype
    n = inp["dx"].size
    named("bits", res["sums"].dtype == dt and bits(res["reduced"])[-1] == bits(res["sums"])[0], "reduced[lr_yy]", res["reduced"][-1], "sums[0]", res["sums"][0])
    if finished:
        named("symmetry", np.array_equal(bits(res["JJ"]), bits(np.ascontiguousarray(res["JJ"].T))), "JJ_out is not bitwise symmetric")
        want = np.abs(res["Jy"]).max()
        named("bits", bits(np.array([res["jy_inf"]], dtype=dt))[0] == bits(np.array([want]))[0], "jy_inf", res["jy_inf"], "max |Jy|", want)
        named("bits", np.array_equal(bits(res["D"][-1]), bits(inp["dx"])), "D[k] is not dx")


def check_same(a, b):
    for key in ("U_col", "D", "JJ", "Jy", "reduced", "partials", "sums"):
        named("bits", np.array_equal(bits(a[key]), bits(b[key])), "a second call changed", key)
    named("bits", bits(np.array([a["jy_inf"]]))[0] == bits(np.array([b["jy_inf"]]))[0], "a second call changed jy_inf")


def check_sums(res, inp):
    """the sums of squares of the count vectors, within gamma_m of the wide sums (entry 0 is held to the sweep's bits elsewhere)"""
    dt = inp["J"].dtype
    W = _wide(dt)
    Y = inp["y"].astype(W)
    ref = np.sum(Y * Y, axis=1)
    m = Y.shape[1]
    err = np.abs(res["sums"].astype(W) - ref)
    named("sums", np.all(err <= _g(m, dt) * ref), "vectors", np.flatnonzero(err > _g(m, dt) * ref))


def check_nogo(res, inp):
    """a record after which no pass follows: every partial entry but lr_yy is +0 (bits), lr_yy holds the sums' bits"""
    p = res["partials"]
    named("nogo", np.all(bits(p[:, :-1]) == 0), "a partial entry other than lr_yy is not +0")
    named("nogo", np.all(bits(res["reduced"][:-1]) == 0), "a reduced entry other than lr_yy is not +0")
    check_bits(res, inp, finished=False)
    check_sums(res, inp)


def check_flush(Jf, inp):
    """flushed J against J0 + U^T D. Exact data: bits. Otherwise J_ij passes k additions and each product its multiplication and
    at most k additions: gamma_{k+1} (|J0| + |U|^T |D|) suffices and gamma_{2k} >= gamma_{k+1} (k >= 1) is the issue's bound; the
    wide reference's gamma_{2k} is added. Returns the largest error / bound."""
    dt = inp["J"].dtype
    k = inp["U"].shape[0]
    ref, ab = wide_flush(inp)
    bound = _g(2 * k, dt) * ab
    err = np.abs(Jf.astype(ref.dtype) - ref)
    named("flush", np.all(err <= bound), "worst error / bound", float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))), "at",
          np.unravel_index(int(np.argmax(err - bound)), err.shape))
    return float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))


def check_exact_flush(Jf, inp):
    ref, ab = wide_flush(inp)
    assert float(ab.max()) < EXACT_LIMIT and np.array_equal(ref, np.rint(ref))
    named("exact", same_bits(Jf, ref.astype(Jf.dtype)), "flushed J at", np.argwhere(Jf != ref.astype(Jf.dtype))[:4].tolist())


def check_chain(JJ, Jy, Jk, y, dtype):
    """JJ, Jy after the chained passes against J_k^T J_k, J_k^T y with J_k = J0 + U^T D in the wide type, under
    jtj_cases.product_bound of |J_k|, |y|: the bound of a product formed afresh. Each pass adds to the error
    u |JJ| for the `+=`, gamma_3 of the term and gamma_m |J0|^T|u| |dx|^T from the sweep; with steps of 0.05 against entries of
    J of order one (random_inputs) four passes stay far inside gamma_m |J_k|^T |J_k|, m = 133."""
    W = _wide(dtype)
    Jw = Jk.astype(W)
    JJr, Jyr = Jw.T @ Jw, Jw.T @ y.astype(W)
    bJJ, bJy = JC.product_bound(Jw, y, dtype)
    eJJ, eJy = np.abs(JJ.astype(W) - JJr), np.abs(Jy.astype(W) - Jyr)
    named("chain", np.all(eJJ <= bJJ), "JJ: worst error / bound", float(np.max(eJJ / bJJ)))
    named("chain", np.all(eJy <= bJy), "Jy: worst error / bound", float(np.max(eJy / bJy)))
    return float(np.max(eJJ / bJJ)), float(np.max(eJy / bJy))


def chain(cell, do_pass, do_flush):
    """passes k = 0 .. CHAIN_PASSES - 1 chained through do_pass (run_pass, or the stand-in), JJ starting as fl(J0^T J0); then
    the identity J_k^T J_k, J_k^T y, then the flush of the four terms. Returns the error / bound ratios."""
    dt = np.dtype(cell.dtype)
    W = _wide(dt)
    m, n = cell.m, cell.n
    base = random_inputs(m, n, 0, dt, seed=100)
    J0, y = base["J"], base["y_old"]
    JJ = (J0.astype(W).T @ J0.astype(W)).astype(dt)
    U, D = np.zeros((0, m), dtype=dt), np.zeros((0, n), dtype=dt)
    for k in range(CHAIN_PASSES):
        step = random_inputs(m, n, 0, dt, seed=101 + k)
        y_old, y = y, (y + 0.1 * step["y_old"]).astype(dt)
        inp = dict(J=J0, U=U, D=D, y=y[None, :], y_old=y_old, JJ=JJ, dx=step["dx"], dx_dot=step["dx_dot"])
        res = do_pass(Cell("pass", cell.dtype, m, n, k, 0, "plain", 1), inp)
        check_u(res, inp)
        check_reduced(res, inp)
        check_finish(res, inp)
        check_bits(res, inp)
        U, D, JJ, Jy = np.concatenate([U, res["U_col"][None, :]]), res["D"], res["JJ"], res["Jy"]
    Jk = J0.astype(W) + U.astype(W).T @ D.astype(W)
    ratios = check_chain(JJ, Jy, Jk, y, dt)
    fin = dict(J=J0, U=U, D=D)
    return ratios + (check_flush(do_flush(Cell("flush", cell.dtype, m, n, CHAIN_PASSES, 0, "", 0), fin), fin),)


# ---------------------------------------------------------------- the device
def _partial(dtype, count, head):
    """a guarded output whose first head.size elements are given and the rest the guard pattern"""
    g = Guarded(dtype, count)
    head = np.ascontiguousarray(head, dtype=dtype).reshape(-1)
    if head.size:
        es = g.dtype.itemsize
        g.buf.upload_at(g.start * es, head.view(UINT[es]))
        g.image[g.start:g.start + head.size] = head.view(UINT[es])
    return g


def run_pass(cell, inp):
    """one mir_lsq_lr_pass on guarded buffers: U of k + 1 columns and D of k + 1 rows (the column / row the pass writes is the last:
    a write behind it lands in the guard). Asserted here: every guard word, J, y, y_old, dx, dx_dot bit-identical, the columns
    < k of U and rows < k of D too, the entry's own bands, state and record; in speculation mode JJ, Jy, D as well, and after a
    record that lets no pass follow the whole of U (column k still the guard pattern)."""
    dt = np.dtype(cell.dtype)
    m, n = inp["J"].shape
    k = inp["U"].shape[0]
    count = inp["y"].shape[0]
    spec = None if cell.mode == "plain" else spec_of(cell.mode, dt)
    go = spec is None or spec_go_by_hand(*spec)
    assert go == (cell.mode not in NOGO)
    gJ = Guarded(dt, m * n, inp["J"], cell.off)
    gU, gD = _partial(dt, (k + 1) * m, inp["U"]), _partial(dt, (k + 1) * n, inp["D"])
    gdx, gdd = Guarded(dt, n, inp["dx"]), Guarded(dt, 1, inp["dx_dot"])
    gy, gyo = Guarded(dt, count * m, inp["y"]), Guarded(dt, m, inp["y_old"])
    gJJ, gJy = Guarded(dt, n * n, inp["JJ"]), Guarded(dt, n)
    kw = {} if spec is None else dict(spec=spec[0], absTolerance=spec[1], relTolerance=spec[2])
    r = api.lrPass(m, n, k, gJ.ptr, gU.ptr, gD.ptr, gdx.ptr, gdd.ptr, gy.ptr, gyo.ptr, gJJ.ptr, gJy.ptr, dtype=dt, count=count, **kw)
    fin = spec is None
    out = {key: g.finish(key, w) for key, g, w in (("J", gJ, False), ("U", gU, go), ("D", gD, fin), ("dx", gdx, False), ("dx_dot", gdd, False),
                                                   ("y", gy, False), ("y_old", gyo, False), ("JJ", gJJ, fin), ("Jy", gJy, fin))}
    named("invariants", r["guard"] == -1 and r["bands"] == 7, "guard band", r["guard"], "of", r["bands"])
    named("invariants", r["touched"] == 0, "state / record written", r["touched"])
    named("invariants", (dt.itemsize, "sweep") + r["cls"] in cell_classes(cell), r["cls"])
    Uo, Do = out["U"].reshape(k + 1, m), out["D"].reshape(k + 1, n)
    named("invariants", np.array_equal(bits(Uo[:k]), bits(inp["U"])), "a column < k of U changed")
    named("invariants", np.array_equal(bits(Do[:k]), bits(inp["D"])), "a row < k of D changed")
    r.update(U_col=Uo[k], D=Do, JJ=out["JJ"].reshape(n, n), Jy=out["Jy"])
    return r


def run_flush(cell, inp):
    """one mir_lsq_lr_flush on guarded buffers: U, D read-only, every guard word intact; -> the flushed J"""
    dt = np.dtype(cell.dtype)
    m, n = inp["J"].shape
    k = inp["U"].shape[0]
    gJ = Guarded(dt, m * n, inp["J"], cell.off)
    gU, gD = Guarded(dt, k * m, inp["U"]), Guarded(dt, k * n, inp["D"])
    cls = api.lrFlush(m, n, k, gJ.ptr, gU.ptr, gD.ptr, dtype=dt)
    out = {key: g.finish(key, w) for key, g, w in (("J", gJ, True), ("U", gU, False), ("D", gD, False))}
    named("invariants", (dt.itemsize, "flush") + cls in cell_classes(cell), cls)
    return out["J"].reshape(m, n)
