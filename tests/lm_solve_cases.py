"""One launch of the LM solve kernels (M.lmSolve -> mir_lsq_lm_solve_d / _s -> launch_lm_solve of csrc/launch_solve.inc) held to
references, at every kernel class: the cells, the problems and points, the references and the named assertions shared by
tests/test_lm_solve_cell_coverage.py (CPU: the cells reach every class, the margin screen, the bounds against a numpy
restatement, the mutation check) and tests/test_gpu_lm_solve.py (the device). Nothing here needs a device but run().

CELLS. (n, dtype, box, generic, one_workgroup): orders NS in both types x box in
  "free"          every bound infinite, the class the driver picks (BOUNDED = false);
  "free_bounded"  every bound infinite, the BOUNDED kernel forced;
  "box"           the family's box (the BOUNDED kernel, asked for as well: run() says why);
7 and 9 in f64 (the wave kernel away from its edges), generic = 1 (the any-n kernel) at n = 16 and 100, and at 257 and 300 the
any-n kernel with its helper workgroups (the driver's width) and on one workgroup. LISTED is the list of instantiated kernel
classes, written out independently of the dispatch; a cell's class comes from the library (api.lm_solve_class, host code).

PROBLEMS. boxqp_cases.family(n, dtype, count=16): J^T J = its P, J^T y = its q, the box its l, u; lambda = LAMBDA = 1 / 8.
POINTS (x rounded to the type).
  "zero"       x = 0: dx is the QP's solution itself and boxqp_cases.check_against_oracle applies unchanged (all 16 problems);
  "inside"     box: the midpoint of a finite interval, a single finite bound -+ 0.5, N(0, 1) without a bound; free: N(0, 1);
  "huge_some"  the inside point with +-HUGE (1e17 in f64, 1e9 in f32) in every third coordinate, whose bounds are made infinite
               (a point outside its box is nothing the solver ever holds): LS:1096-1097 round those steps to zero;
  "huge_all"   +-HUGE everywhere. Only with every bound infinite ("free", "free_bounded": both BOUNDED instances). A null step
               where every |xq_i| stays below half the spacing at HUGE (8 in f64, 32 in f32): the small orders;
  "null"       +-NULL_X (2^80 in f64, 2^50 in f32) everywhere, bounds as for "huge_all": a null step at every order.
The last four on four problems each.

REFERENCE. The QP of a launch is P = J^T J with fl(JJ_ii + lambda) on the diagonal, q = J^T y, fl(l - x), fl(u - x), solved by
oracle.solve_box_qp in the type and in f64. Everything else is written out below in numpy: in the type where bits are claimed, in
longdouble where a bound is claimed (u = eps / 2, gamma_k = k u / (1 - k u)).

ASSERTIONS (each raises AssertionError("<name>: ...")); the GPU file's docstring has what the kernels need of each bound.
  solve       x = 0: check_against_oracle with SINGLE_MARGIN; elsewhere the status and
              |dx - fl(fl(x64 + x) - x)| <= x_tolerance + ulp(|x| + |dx|), x64 the f64 oracle's solution
  trial       trial == fmax(fmin(fl(dx + x), upper), lower), bits
  flags       null step iff all(trial == x); NaN flags iff a NaN is there; step guard iff !(sqrt(new_dx_dot) < maxStep)
  new_dx_dot  within gamma_{n+1} sum dx^2 of sum dx^2
  predicted   within gamma_{n+3} sum_i (sum_j |JJ_ij| |dx_j| + 2 |Jy_i|) |dx_i| of -dx^T (JJ dx + 2 Jy), JJ UNDAMPED
  trial_xnorm within gamma_{n+8} ||trial||_2 of ||trial||_2
  lambda0     the record's lambda is T(0.001) * JJ[f][f], f the FIRST index of maximum |diagonal|; 1 when that is below minLambda
  gradient    jy_inf == max |Jy|; not (jy_inf > gradTolerance): flags == 16, every other field 0, dx / trial untouched
  ladder      entry k of a launch of 8 == the launch of lam[k] alone, bits; rows >= ks untouched
  invariants  inputs back bit-identical, every guard band intact, the class the cell names
These gamma are first-order bounds of the operation counts, not measurements: the products (1 rounding each), a sum of n terms in
any order (n - 1), + 2 Jy, * dx, the final sum's tree; the norm's division, square, sum, square root (correctly rounded) and
product. The restatement below stays inside them in three summation orders (CPU tier).
"""
import collections

import numpy as np

import mir_optim_amd as M
from mir_optim_amd import api
import boxqp_cases as B

COUNT = B.SINGLE_COUNT
NS = (1, 2, 15, 16, 17, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 300)
NS_F64_EXTRA = (7, 9)
GENERIC_NS = (16, 100)
BIG_NS = (257, 300)
BOXES = ("free", "free_bounded", "box")
DTYPES = (np.float32, np.float64)
LAMBDA = 0.125
HUGE = {np.float32: 1e9, np.float64: 1e17}
NULL_X = {np.float32: 2.0 ** 50, np.float64: 2.0 ** 80}
POINTS = ("zero", "inside", "huge_some", "huge_all", "null")
FEW = 4                                  # problems of the points other than "zero"
LADDER = tuple(0.125 * 10.0 ** k * 2.0 ** (k * (k - 1) // 2) for k in range(8))    # LS:1103-1104 with lambdaIncrease = 10

Cell = collections.namedtuple("Cell", "n dtype box generic one_workgroup")


def _cells():
    out = []
    for dt in DTYPES:
        for n in NS + (NS_F64_EXTRA if dt == np.float64 else ()):
            out += [Cell(n, dt, box, False, False) for box in BOXES]
        out += [Cell(n, dt, box, True, False) for n in GENERIC_NS for box in ("free", "box")]
        out += [Cell(n, dt, box, False, True) for n in BIG_NS for box in ("free", "box")]
    return tuple(out)


CELLS = _cells()


def cell_id(c):
    return (f"{np.dtype(c.dtype).name}-n{c.n}-{c.box}" + ("-generic" if c.generic else "") + ("-one_workgroup" if c.one_workgroup else ""))


def cell_class(c):
    """(element size, kind, LDS blocks a side, BOUNDED) of the kernel the cell's launches run, by the library's own dispatch"""
    return (np.dtype(c.dtype).itemsize,) + api.lm_solve_class(np.dtype(c.dtype).itemsize, c.n, c.box != "free", c.generic)


# every instance launch_solve_d.hip / launch_solve_s.hip compile, written out by hand: (element size, kind, NB, BOUNDED)
LISTED = {}
for _b in (False, True):
    LISTED[(8, "wave", 0, _b)] = "run"
    for _nb in (1, 2, 4, 8, 0):
        LISTED[(4, "workgroup", _nb, _b)] = "run"
    for _nb in (2, 4, 8, 0):
        LISTED[(8, "workgroup", _nb, _b)] = "run"
    LISTED[(8, "workgroup", 1, _b)] = "not run: n <= 16 in f64 reaches it only with the diagnostic buffer attached"
LISTED[(4, "big", 0, True)] = "run"
LISTED[(8, "big", 0, True)] = "run"


def has_copy_loop(key):
    """the J^T J copy loop of lm_solve_body (its even-n^2 and odd-n^2 branches): NB == 0 or BOUNDED, workgroup kernels"""
    return key[1] == "workgroup" and (key[2] == 0 or key[3])


# ---------------------------------------------------------------- problems, points, the oracle's answers
def as_t(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def problem(n, dtype, box, p):
    P, q, l, u = B.family(n, dtype, count=COUNT)
    if box != "box":
        return P[p], q[p], np.full(n, -np.inf), np.full(n, np.inf)
    return P[p], q[p], l[p], u[p]


def point(name, n, dtype, box, p):
    """(x, lower, upper) of problem p at the named point, float64 arrays of values of the type"""
    _, _, l, u = problem(n, dtype, box, p)
    rng = np.random.default_rng([20261, n, p])
    z = rng.standard_normal(n)
    if name == "zero":
        return np.zeros(n), l, u
    lf, uf = np.isfinite(l), np.isfinite(u)
    with np.errstate(invalid="ignore"):
        x = np.where(lf & uf, (np.nan_to_num(l) + np.nan_to_num(u)) / 2, np.where(lf, l + 0.5, np.where(uf, u - 0.5, z)))
    x = np.clip(x.astype(dtype).astype(np.float64), l, u)
    if name == "inside":
        return x, l, u
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    big = (HUGE[dtype] * sign).astype(dtype).astype(np.float64)
    if name in ("huge_all", "null"):
        assert box != "box"
        return (big if name == "huge_all" else NULL_X[dtype] * sign), l, u
    S = np.arange(n) % 3 == 0
    return np.where(S, big, x), np.where(S, -np.inf, l), np.where(S, np.inf, u)


def point_problems(name, box):
    if name == "zero":
        return tuple(range(COUNT))
    if name in ("huge_all", "null") and box == "box":
        return ()
    return tuple(range(FEW))


def qp_of(JJ, x, l, u, lam, dtype):
    """P = JJ with fl(JJ_ii + lambda) on the diagonal, fl(l - x), fl(u - x): float64 arrays of values of the type"""
    T = np.dtype(dtype).type
    Pl = as_t(JJ, dtype).copy()
    i = np.arange(len(x))
    Pl[i, i] = Pl[i, i] + T(lam)
    with np.errstate(over="ignore", invalid="ignore"):
        ql, qu = as_t(l, dtype) - as_t(x, dtype), as_t(u, dtype) - as_t(x, dtype)
    return Pl.astype(np.float64), ql.astype(np.float64), qu.astype(np.float64)


_REF = {}


def reference(oracle, n, dtype, box, name, lam=LAMBDA):
    """what the launches of (n, dtype, box) at a point are compared with, computed once and shared (read-only): the problems idx,
    their x, l, u, the QP (P, q, ql, qu), the oracle's answers in the type and in f64 and the margin screen"""
    key = (n, np.dtype(dtype).name, "box" if box == "box" else "free", name, lam)
    if key not in _REF:
        idx = point_problems(name, box)
        JJ, Jy, X, Lo, Up, Pl, Ql, Qu = ([] for _ in range(8))
        for p in idx:
            P, q, _, _ = problem(n, dtype, box, p)
            x, l, u = point(name, n, dtype, box, p)
            pl, ql, qu = qp_of(P, x, l, u, lam, dtype)
            for lst, v in zip((JJ, Jy, X, Lo, Up, Pl, Ql, Qu), (P, q, x, l, u, pl, ql, qu)):
                lst.append(v)
        r = {k: np.stack(v) for k, v in zip(("JJ", "Jy", "x", "l", "u", "P", "ql", "qu"), (JJ, Jy, X, Lo, Up, Pl, Ql, Qu))}
        r["idx"] = np.array(idx)
        r["ora"] = B.oracle_solve(oracle, r["P"], r["Jy"], r["ql"], r["qu"], dtype)
        r["ora64"] = B.oracle_solve(oracle, r["P"], r["Jy"], r["ql"], r["qu"], np.float64)
        s64, x64, _ = r["ora64"]
        r["screened"] = np.array([s64[k] == 0 and B.margin_screened(r["P"][k], r["Jy"][k], r["ql"][k], r["qu"][k], x64[k],
                                                                     B.SINGLE_MARGIN[dtype]) for k in range(len(idx))])
        for v in r.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


# ---------------------------------------------------------------- the numpy restatement (the stand-in of the kernels)
def gamma(k, dtype):
    u = np.longdouble(np.finfo(dtype).eps) / 2
    return k * u / (1 - k * u)


def tsum(v, order, axis=-1):
    """sum in v's own type: 0 left to right, 1 numpy's pairwise sum, 2 right to left"""
    v = np.asarray(v)
    if v.shape[axis] == 0:
        return np.zeros(v.shape[:-1], dtype=v.dtype)
    if order == 1:
        return v.sum(axis=axis, dtype=v.dtype)
    if order == 2:
        v = np.flip(v, axis=axis)
    return np.take(np.add.accumulate(v, axis=axis, dtype=v.dtype), -1, axis=axis)


def settings_values(settings):
    return {k: getattr(settings, k) for k in ("gradTolerance", "minLambda", "maxStep")}


def lambda0_tie(JJ):
    """-d at index 0 and +d at the last one, d twice the largest |diagonal entry|: the FIRST entry of maximum modulus gives
    lambda_0 = -0.001 d, below minLambda, so 1; the largest entry, or the last maximum, would give 0.001 d"""
    JJ = JJ.copy()
    d = 2 * np.abs(np.diagonal(JJ)).max()
    JJ[0, 0], JJ[-1, -1] = -d, d
    return JJ


def standin_lambda0(JJ, state_lambda, min_lambda, dtype, mutate=None):
    """LS:1067-1072 on entry 0 of a launch with lambda_from_state"""
    T = np.dtype(dtype).type
    lam = T(state_lambda)
    if lam >= T(min_lambda):
        return lam
    d = as_t(np.diagonal(JJ), dtype)
    ad = np.abs(d)
    hits = np.flatnonzero(ad == ad.max())
    f = hits[-1] if mutate == "lambda0_last" else hits[0]
    lam = T(0.001) * d[f]
    return lam if lam >= T(min_lambda) else T(1)


def standin_epilogue(xq, JJ, Jy, x, l, u, lam, dtype, max_step, order=0, mutate=None):
    """LS:1087-1110, 1141-1142, 1164 from the QP's solution xq, in the type: (dx, trial, new_dx_dot, predicted, trial_xnorm, flags)"""
    T = np.dtype(dtype).type
    xq, JJ, Jy, x, l, u = (as_t(a, dtype) for a in (xq, JJ, Jy, x, l, u))
    with np.errstate(over="ignore", invalid="ignore"):
        d = (xq + x) - x
        tr = d + x if mutate == "unclamped" else np.fmax(np.fmin(d + x, u), l)
        flags = (api.LM_FLAG_DX_NAN if np.isnan(xq).any() else 0) | (api.LM_FLAG_X_NAN if np.isnan(tr).any() else 0)
        if np.all(tr == x):
            flags |= api.LM_FLAG_NULL_STEP
        dd = xq if mutate == "unrounded_ndd" else d
        ndd = tsum(dd * dd, order)
        Mx = JJ.copy()
        i = np.arange(len(x))
        if mutate == "damped":
            Mx[i, i] = Mx[i, i] + T(lam)
        if mutate == "no_diag":
            Mx[i, i] = 0
        t = tsum(Mx * d[None, :], order) + T(2) * Jy
        pred = -tsum(t * d, order)
        amx = np.abs(tr).max()
        xn = amx * np.sqrt(tsum((tr / amx) ** 2, order)) if amx > 0 else T(0)
        if not np.sqrt(ndd) < T(max_step):
            flags |= api.LM_FLAG_STEP_TOO_LONG
    return d, tr, ndd, pred, xn, flags


def standin_launch(oracle, JJ, Jy, x, l, u, lams, dtype, settings=None, state_lambda=0.0, check_grad=False, lambda_from_state=False,
                   order=0, mutate=None):
    """what M.lmSolve returns, from oracle.solve_box_qp and the restatement above (rec, dx, trial, jy_inf)"""
    T = np.dtype(dtype).type
    sv = settings_values(settings or M.LeastSquaresSettings(dtype))
    n, ks = len(x), len(lams)
    rec = np.zeros(ks, dtype=api.lm_solve_record_dtype(dtype))
    dx = np.full((api.LM_SOLVE_CHAIN, n), api.LM_SOLVE_SENTINEL, dtype=dtype)
    trial = dx.copy()
    jy_inf = T(0)
    if check_grad:
        jy_inf = np.abs(as_t(Jy, dtype)).max()
        if not jy_inf > T(sv["gradTolerance"]):
            rec["flags"][:] = api.LM_FLAG_GRAD_SMALL
            return {"rec": rec, "dx": dx, "trial": trial, "jy_inf": jy_inf}
    for k in range(ks):
        lam = T(lams[k - 1] if (mutate == "ladder_prev" and k > 0) else lams[k])
        if k == 0 and lambda_from_state:
            lam = standin_lambda0(JJ, state_lambda, sv["minLambda"], dtype, mutate)
        Pl, ql, qu = qp_of(JJ, x, l, u, lam, dtype)
        st, xq, it = oracle.solve_box_qp(np.tril(Pl), Jy, ql, qu, dtype=dtype)
        rec[k]["lambda"], rec[k]["qp_status"], rec[k]["qp_iterations"] = lam, st, it
        if st == 0:
            d, tr, ndd, pred, xn, flags = standin_epilogue(xq, JJ, Jy, x, l, u, lam, dtype, sv["maxStep"], order, mutate)
            dx[k], trial[k] = d, tr
            rec[k]["new_dx_dot"], rec[k]["predicted"], rec[k]["trial_xnorm"], rec[k]["flags"] = ndd, pred, xn, flags
    return {"rec": rec, "dx": dx, "trial": trial, "jy_inf": jy_inf}


# ---------------------------------------------------------------- the named assertions
def named(name, ok, *what):
    if not ok:
        raise AssertionError(f"{name}: " + " ".join(str(w) for w in what))


def untouched(a):
    return bool(np.all(a == a.dtype.type(api.LM_SOLVE_SENTINEL)))


def check_epilogue(res, k, JJ, Jy, x, l, u, dtype, max_step):
    """the record, dx and trial of ladder entry k (qp_status 0) against the restatement from the device's own dx; returns the
    error / bound ratios of new_dx_dot, predicted, trial_xnorm"""
    rec, dx, trial = res["rec"][k], res["dx"][k], res["trial"][k]
    T = np.dtype(dtype).type
    n = len(x)
    JJt, Jyt, xt, lt, ut = (as_t(a, dtype) for a in (JJ, Jy, x, l, u))
    named("trial", dx.dtype == dtype and trial.dtype == dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        want = np.fmax(np.fmin(dx + xt, ut), lt)
    named("trial", np.array_equal(B.bits(trial), B.bits(want)), "not clip(fl(dx + x), lower, upper) at", np.flatnonzero(B.bits(trial) != B.bits(want))[:4])
    fl = int(rec["flags"])
    named("flags", bool(fl & api.LM_FLAG_NULL_STEP) == bool(np.all(trial == xt)), "null step", fl)
    named("flags", bool(fl & api.LM_FLAG_DX_NAN) == bool(np.isnan(dx).any()), "NaN in dx", fl)
    named("flags", bool(fl & api.LM_FLAG_X_NAN) == bool(np.isnan(trial).any()), "NaN in trial", fl)
    named("flags", bool(fl & api.LM_FLAG_STEP_TOO_LONG) == (not np.sqrt(T(rec["new_dx_dot"])) < T(max_step)), "step guard", fl, rec["new_dx_dot"], max_step)
    named("flags", fl & ~(api.LM_FLAG_NULL_STEP | api.LM_FLAG_DX_NAN | api.LM_FLAG_X_NAN | api.LM_FLAG_STEP_TOO_LONG | api.LM_FLAG_COOP_RESCUED) == 0, fl)
    L = np.longdouble
    d, A, g, tr = dx.astype(L), JJt.astype(L), Jyt.astype(L), trial.astype(L)
    ratios = {}
    exact = np.sum(d * d)
    bound = gamma(n + 1, dtype) * exact
    err = abs(L(rec["new_dx_dot"]) - exact)
    ratios["new_dx_dot"] = float(err / bound) if bound > 0 else 0.0
    named("new_dx_dot", err <= bound, float(err), float(bound))
    exact = -np.sum(d * (A @ d + 2 * g))
    bound = gamma(n + 3, dtype) * np.sum((np.abs(A) @ np.abs(d) + 2 * np.abs(g)) * np.abs(d))
    err = abs(L(rec["predicted"]) - exact)
    ratios["predicted"] = float(err / bound) if bound > 0 else 0.0
    named("predicted", err <= bound, float(rec["predicted"]), float(exact), float(err), float(bound))
    amx = np.abs(tr).max()
    exact = amx * np.sqrt(np.sum((tr / amx) ** 2)) if amx > 0 else L(0)
    bound = gamma(n + 8, dtype) * exact
    err = abs(L(rec["trial_xnorm"]) - exact)
    ratios["trial_xnorm"] = float(err / bound) if bound > 0 else 0.0
    named("trial_xnorm", err <= bound, float(rec["trial_xnorm"]), float(exact), float(err), float(bound))
    return ratios


def ulp(v, dtype):
    return np.spacing(np.abs(as_t(v, dtype))).astype(np.float64)


def check_step(dx, x, x64, tol, dtype):
    """|dx - fl(fl(x64 + x) - x)| <= x_tolerance + ulp(|x| + |dx|) for one problem away from x = 0"""
    xt = as_t(x, dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        want = ((as_t(x64, dtype) + xt) - xt).astype(np.float64)
    allow = tol + ulp(np.abs(x) + np.abs(dx.astype(np.float64)), dtype)
    dist = np.abs(dx.astype(np.float64) - want)
    named("solve", np.all(dist <= allow), "step", float(np.max(dist / allow)))
    return float(np.max(dist / allow))


def check_lambda0(res, JJ, state_lambda, settings, dtype):
    want = standin_lambda0(JJ, state_lambda, settings_values(settings)["minLambda"], dtype)
    got = res["rec"][0]["lambda"]
    named("lambda0", got.dtype == np.dtype(dtype) and B.bits(np.array([got]))[0] == B.bits(np.array([want]))[0], float(got), float(want))


def check_gradient(res, Jy, grad_tolerance, dtype):
    T = np.dtype(dtype).type
    want = np.abs(as_t(Jy, dtype)).max()
    named("gradient", B.bits(np.array([res["jy_inf"]], dtype=dtype))[0] == B.bits(np.array([want]))[0], "jy_inf", float(res["jy_inf"]), float(want))
    small = not want > T(grad_tolerance)
    rec = res["rec"][0]
    named("gradient", bool(rec["flags"] & api.LM_FLAG_GRAD_SMALL) == small, "flag", int(rec["flags"]), small)
    if small:
        zero = np.zeros(1, dtype=res["rec"].dtype)[0]
        zero["flags"] = api.LM_FLAG_GRAD_SMALL
        named("gradient", rec.tobytes() == zero.tobytes(), "record", rec)
        named("gradient", untouched(res["dx"]) and untouched(res["trial"]), "dx / trial written")
    return small


def same_entry(a, ka, b, kb):
    return (a["rec"][ka].tobytes() == b["rec"][kb].tobytes() and a["dx"][ka].tobytes() == b["dx"][kb].tobytes()
            and a["trial"][ka].tobytes() == b["trial"][kb].tobytes())


def check_ladder(full, singles):
    """entry k of the launch of len(singles) entries against the launch of its lambda alone; rows behind the ladder untouched"""
    ks = len(singles)
    for k in range(ks):
        named("ladder", same_entry(full, k, singles[k], 0), "entry", k, full["rec"][k], singles[k]["rec"][0])
    named("ladder", untouched(full["dx"][ks:]) and untouched(full["trial"][ks:]), "rows behind the ladder written")
    for s in singles:
        named("ladder", untouched(s["dx"][1:]) and untouched(s["trial"][1:]), "rows behind a ladder of one written")


def check_invariants(res, given, cell=None):
    """inputs back bit-identical, guard bands intact, the class and helper width the cell names"""
    for a, b in zip(res["inputs"], given):
        named("invariants", np.array_equal(B.bits(a), B.bits(as_t(b, a.dtype))), "an input changed")
    named("invariants", res["guard"] == -1, "guard band", res["guard"], "of", res["bands"], "damaged")
    named("invariants", res["bands"] == 9 + 7 * api.LM_SOLVE_CHAIN + 1, res["bands"])
    if cell is not None:
        named("invariants", (np.dtype(cell.dtype).itemsize,) + res["cls"] == cell_class(cell), res["cls"], cell_class(cell))
        if cell.n <= 256 or cell.one_workgroup:
            named("invariants", res["helpers"] == 1, res["helpers"])
        else:
            named("invariants", res["helpers"] == min((((cell.n + 15) // 16 + 3) // 4), 16) and res["helpers"] >= 2, res["helpers"])


# ---------------------------------------------------------------- the device
def run(cell, JJ, Jy, x, l, u, lams=(LAMBDA,), **kw):
    """one launch for the cell (generic / one_workgroup as the cell says), invariants asserted. Only "free" leaves the choice of
    the BOUNDED instance to the driver's rule; "box" asks for it as "free_bounded" does, which changes nothing while a bound is
    finite and keeps the cell on its class where a point has made every bound infinite (n = 1 at "huge_some")"""
    res = M.lmSolve(JJ, Jy, x, l, u, lams, dtype=cell.dtype, force_bounded=cell.box != "free", generic=cell.generic,
                    one_workgroup=cell.one_workgroup, **kw)
    check_invariants(res, (JJ, Jy, x, l, u), cell)
    ks = len(lams)
    named("ladder", untouched(res["dx"][ks:]) and untouched(res["trial"][ks:]), "rows behind the ladder written")
    return res


def writes_on_failure(cell):
    """k_lm_solve_wave stores dx / trial of an entry whenever the gradient test passes (its epilogue is unconditional); the
    workgroup kernels and the any-n kernel only when the QP ended with status 0"""
    return cell_class(cell)[1] == "wave"
