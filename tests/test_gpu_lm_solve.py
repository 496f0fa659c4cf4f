"""The LM solve kernels one launch at a time (M.lmSolve -> mir_lsq_lm_solve_d / _s -> launch_lm_solve: k_lm_solve_wave<BOUNDED>,
k_lm_solve<T, NB, BOUNDED>, k_lm_solve_big<T> with and without helper workgroups) against references, at every instantiated
class: the cells, points, references and named assertions are tests/lm_solve_cases.py's (its docstring has the rules and the
bounds; tests/test_lm_solve_cell_coverage.py keeps on the CPU that the cells reach every class and that the assertions catch
planted mistakes). One family of 16 problems a cell at x = 0, four problems at each other point, each call one launch between
guard bands; every launch also asserts that its inputs come back bit-identical, that every guard band is intact and that the
class and helper width are the ones the cell names.

What a failed QP leaves behind differs between the classes and is asserted as it is: the workgroup kernels and the any-n
kernel write dx / trial only when the QP ended with status 0; k_lm_solve_wave runs its epilogue unconditionally and stores both
rows whenever the gradient test passed (the round's decision reads neither after a failed QP).

Measured on an MI355X with this file: 979 tests in 15.5 s (the slowest, a family of 16 at n = 256 / 300, 0.25 s). Largest
error / bound over every cell, point and ladder entry of a class (new_dx_dot / predicted / trial_xnorm; then the largest
distance of dx from the f64 oracle's rounded step over its allowance, away from x = 0):
  class (orders run)                          float32                          float64
  k_lm_solve_wave<false> (1 .. 16)            --                               0.41 / 0.24 / 0.15;  0.14
  k_lm_solve_wave<true>                       --                               0.43 / 0.24 / 0.15;  0.14
  k_lm_solve<NB=1, false> (1, 2, 15, 16)      0.42 / 0.17 / 0.16;  0.57        (diagnostic buffer only: not run)
  k_lm_solve<NB=1, true>                      0.46 / 0.22 / 0.17;  0.57        (not run)
  k_lm_solve<NB=2, false> (17, 32)            0.06 / 0.05 / 0.08;  0.57        0.10 / 0.06 / 0.05;  0.03
  k_lm_solve<NB=2, true>                      0.10 / 0.08 / 0.08;  0.57        0.11 / 0.06 / 0.05;  0.03
  k_lm_solve<NB=4, false> (33, 64)            0.05 / 0.03 / 0.03;  0.33        0.05 / 0.05 / 0.03;  0.04
  k_lm_solve<NB=4, true>                      0.05 / 0.03 / 0.05;  0.37        0.05 / 0.05 / 0.04;  0.04
  k_lm_solve<NB=8, false> (65, 127, 128)      0.02 / 0.02 / 0.02;  0.23        0.03 / 0.01 / 0.02;  0.04
  k_lm_solve<NB=8, true>                      0.02 / 0.02 / 0.02;  0.42        0.03 / 0.02 / 0.02;  0.04
  k_lm_solve<NB=0, false> (129, 255, 256)     0.02 / 0.01 / 0.01;  0.29        0.01 / 0.01 / 0.01;  0.06
  k_lm_solve<NB=0, true>                      0.02 / 0.01 / 0.01;  0.29        0.01 / 0.01 / 0.01;  0.06
  k_lm_solve_big, one workgroup (16*, 100*,   0.09 / 0.05 / 0.06;  0.35        0.10 / 0.06 / 0.07;  0.08
    257, 300)
  k_lm_solve_big with helpers (257, 300)      0.01 / 0.01 / 0.01;  0.28        0.01 / 0.01 / 0.01;  0.06
(* generic = 1: those orders run the any-n kernel.) No class comes near a bound; the largest ratios are those of n = 1, 2, where
the bound is two or three roundings wide. The numpy restatement's own ratios (CPU tier) are of the same size: 0.46 / 0.21 / 0.15
at n <= 2, 0.03 / 0.004 / 0.02 at n = 300.

One defect showed, in a field nobody reads: after a failed gradient test k_lm_solve_wave left the lambda it had been handed in
the record (0.125 here) where every other class leaves 0 -- test_gradient_test failed on all f64 cells with n <= 16 with
"gradient: record (0.125, 0.0, 0.0, 0.0, 0, 0, 16, 0)"; the kernel now writes 0 there.
"""
import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api
import boxqp_cases as B
import lm_solve_cases as K

pytestmark = pytest.mark.gpu

CELL = [pytest.param(c, id=K.cell_id(c)) for c in K.CELLS]
FORCED = [pytest.param(c, id=K.cell_id(c)) for c in K.CELLS if c.box == "free_bounded"]
_DEVICE = {}
WORST = {}


def launches(oracle, cell, name):
    """the cell's launches at a point with default settings and lambda = LAMBDA, made once and shared (read-only)"""
    key = (cell, name)
    if key not in _DEVICE:
        r = K.reference(oracle, cell.n, cell.dtype, cell.box, name)
        out = []
        for k in range(len(r["idx"])):
            res = K.run(cell, r["JJ"][k], r["Jy"][k], r["x"][k], r["l"][k], r["u"][k])
            del res["inputs"]
            out.append(res)
        _DEVICE[key] = out
    return _DEVICE[key]


def note(cell, ratios):
    w = WORST.setdefault(K.cell_class(cell) + (("helpers",) if cell.n > 256 and not cell.one_workgroup else ()), {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), v)


def epilogue(cell, res, r, k, max_step=None, entry=0):
    s = M.LeastSquaresSettings(cell.dtype)
    ratios = K.check_epilogue(res, entry, r["JJ"][k], r["Jy"][k], r["x"][k], r["l"][k], r["u"][k], cell.dtype,
                              s.maxStep if max_step is None else max_step)
    note(cell, ratios)


def oracle_status(oracle, JJ, Jy, x, l, u, lam, dtype):
    Pl, ql, qu = K.qp_of(JJ, x, l, u, lam, dtype)
    return oracle.solve_box_qp(np.tril(Pl), Jy, ql, qu, dtype=dtype)


# ---------------------------------------------------------------- 1, 2: the solve and the epilogue at every point
@pytest.mark.parametrize("cell", CELL)
def test_family_at_x_zero(oracle, cell):
    r = K.reference(oracle, cell.n, cell.dtype, cell.box, "zero")
    res = launches(oracle, cell, "zero")
    dev = (np.array([a["rec"][0]["qp_status"] for a in res]), np.stack([a["dx"][0] for a in res]),
           np.array([a["rec"][0]["qp_iterations"] for a in res]))
    B.check_against_oracle(dev, r["ora"], r["ora64"], (r["P"], r["Jy"], r["ql"], r["qu"]), cell.dtype, r["screened"])
    T = np.dtype(cell.dtype).type
    for k, a in enumerate(res):
        assert a["rec"][0]["lambda"] == T(K.LAMBDA) and a["rec"][0]["reserved"] == 0 and a["jy_inf"] == 0
        if a["rec"][0]["qp_status"] == 0:
            epilogue(cell, a, r, k)
            assert not a["rec"][0]["flags"] & api.LM_FLAG_STEP_TOO_LONG
        else:
            assert K.writes_on_failure(cell) or (K.untouched(a["dx"]) and K.untouched(a["trial"]))


@pytest.mark.parametrize("cell", CELL)
def test_points_away_from_zero(oracle, cell):
    for name in K.POINTS[1:]:
        if not K.point_problems(name, cell.box):
            continue
        r = K.reference(oracle, cell.n, cell.dtype, cell.box, name)
        res = launches(oracle, cell, name)
        so, xo, _ = r["ora"]
        s64, x64, _ = r["ora64"]
        assert np.array_equal([a["rec"][0]["qp_status"] for a in res], so), name
        tol = B.x_tolerance(cell.dtype, r["P"], x64, xo)
        for k, a in enumerate(res):
            if so[k] != 0 or s64[k] != 0:
                continue
            ratio = K.check_step(a["dx"][0], r["x"][k], x64[k], tol[k], cell.dtype)
            note(cell, {"step": ratio})
            epilogue(cell, a, r, k)
            null = bool(a["rec"][0]["flags"] & api.LM_FLAG_NULL_STEP)
            if name == "null":
                assert null and a["rec"][0]["new_dx_dot"] == 0 and a["rec"][0]["predicted"] == 0 and not a["dx"][0].any()
            if name == "inside":
                assert not null
            if name == "huge_some":
                S = np.arange(cell.n) % 3 == 0
                assert np.all(a["dx"][0][S] % np.spacing(cell.dtype(K.HUGE[cell.dtype])) == 0)


@pytest.mark.parametrize("cell", CELL)
def test_a_second_call_gives_the_same_bits(oracle, cell):
    for name in ("zero", "inside"):
        r = K.reference(oracle, cell.n, cell.dtype, cell.box, name)
        first = launches(oracle, cell, name)[0]
        again = K.run(cell, r["JJ"][0], r["Jy"][0], r["x"][0], r["l"][0], r["u"][0])
        assert K.same_entry(again, 0, first, 0), name


# ---------------------------------------------------------------- 3: lambda_0
@pytest.mark.parametrize("cell", CELL)
def test_lambda0_rule(oracle, cell):
    dtype = cell.dtype
    T = np.dtype(dtype).type
    r = K.reference(oracle, cell.n, dtype, cell.box, "inside")
    JJ, Jy, x, l, u = (r[k][0] for k in ("JJ", "Jy", "x", "l", "u"))
    s = M.LeastSquaresSettings(dtype)
    half = M.LeastSquaresSettings(dtype)
    half.minLambda = 0.5
    cases = [("default", JJ, s, 0.0, None), ("below minLambda", JJ, half, 0.0, T(1)), ("state taken", JJ, s, 0.25, T(0.25))]
    if cell.n >= 2:
        cases.append(("tie", K.lambda0_tie(JJ), s, 0.0, T(1)))
    for what, A, st, state, want in cases:
        res = K.run(cell, A, Jy, x, l, u, lams=(7.0,), settings=st, state_lambda=state, lambda_from_state=True)
        K.check_lambda0(res, A, state, st, dtype)
        lam = res["rec"][0]["lambda"]
        if want is not None:
            assert lam == want, (what, lam)
        so, _, io = oracle_status(oracle, A, Jy, x, l, u, lam, dtype)
        assert res["rec"][0]["qp_status"] == so, (what, res["rec"][0], so)
        if so == 0:                                        # (the tie's J^T J + I is indefinite wherever d > 1: the oracle's word)
            K.check_epilogue(res, 0, A, Jy, x, l, u, dtype, st.maxStep)
    # without lambda_from_state the state's lambda is not read
    res = K.run(cell, JJ, Jy, x, l, u, lams=(K.LAMBDA,), state_lambda=0.25)
    assert K.same_entry(res, 0, launches(oracle, cell, "inside")[0], 0)


# ---------------------------------------------------------------- 4: the gradient test
@pytest.mark.parametrize("cell", CELL)
def test_gradient_test(oracle, cell):
    dtype = cell.dtype
    T = np.dtype(dtype).type
    r = K.reference(oracle, cell.n, dtype, cell.box, "inside")
    JJ, Jy, x, l, u = (r[k][0] for k in ("JJ", "Jy", "x", "l", "u"))
    g = np.abs(Jy.astype(dtype)).max()
    plain = launches(oracle, cell, "inside")[0]
    for tol, small in ((g, True), (np.nextafter(g, T(np.inf)), True), (np.nextafter(g, T(0)), False)):
        s = M.LeastSquaresSettings(dtype)
        s.gradTolerance = float(tol)
        res = K.run(cell, JJ, Jy, x, l, u, settings=s, check_grad=True)
        assert K.check_gradient(res, Jy, s.gradTolerance, dtype) == small
        if not small:
            assert K.same_entry(res, 0, plain, 0)


# ---------------------------------------------------------------- 5: the ladder
@pytest.mark.parametrize("cell", CELL)
def test_ladder_entries_are_the_single_launches(oracle, cell):
    r = K.reference(oracle, cell.n, cell.dtype, cell.box, "inside")
    JJ, Jy, x, l, u = (r[k][0] for k in ("JJ", "Jy", "x", "l", "u"))
    full = K.run(cell, JJ, Jy, x, l, u, lams=K.LADDER)
    singles = [K.run(cell, JJ, Jy, x, l, u, lams=(lam,)) for lam in K.LADDER]
    K.check_ladder(full, singles)
    assert K.same_entry(singles[0], 0, launches(oracle, cell, "inside")[0], 0)
    for k in range(len(K.LADDER)):
        assert full["rec"][k]["qp_status"] == 0 and full["rec"][k]["lambda"] == np.dtype(cell.dtype).type(K.LADDER[k])
        epilogue(cell, full, {key: r[key][:1] for key in ("JJ", "Jy", "x", "l", "u")}, 0, entry=k)


# ---------------------------------------------------------------- 2 (step guard), 6: failures
@pytest.mark.parametrize("cell", CELL)
def test_step_guard(oracle, cell):
    """maxStep a factor 2 either side of ||dx||: the rounding of the square root cannot decide it"""
    r = K.reference(oracle, cell.n, cell.dtype, cell.box, "inside")
    JJ, Jy, x, l, u = (r[k][0] for k in ("JJ", "Jy", "x", "l", "u"))
    plain = launches(oracle, cell, "inside")[0]
    norm = float(np.sqrt(np.sum(plain["dx"][0].astype(np.float64) ** 2)))
    assert norm > 0
    for factor, long in ((2.0, False), (0.5, True)):
        s = M.LeastSquaresSettings(cell.dtype)
        s.maxStep = factor * norm
        res = K.run(cell, JJ, Jy, x, l, u, settings=s)
        K.check_epilogue(res, 0, JJ, Jy, x, l, u, cell.dtype, s.maxStep)
        assert bool(res["rec"][0]["flags"] & api.LM_FLAG_STEP_TOO_LONG) == long
        res["rec"]["flags"] &= ~api.LM_FLAG_STEP_TOO_LONG
        assert K.same_entry(res, 0, plain, 0)


@pytest.mark.parametrize("cell", CELL)
def test_failures_give_the_oracles_status(oracle, cell):
    n, dtype = cell.n, cell.dtype
    r = K.reference(oracle, n, dtype, cell.box, "inside")
    JJ, Jy, x, l, u = (r[k][0] for k in ("JJ", "Jy", "x", "l", "u"))
    nan = JJ.copy()
    nan[n - 1, 0] = nan[0, n - 1] = np.nan
    bad = [("NaN", nan)] + [(f"indefinite at {k}", B.indefinite(JJ, k)) for k in sorted({0, n - 1})]
    for what, A in bad:
        so, _, io = oracle_status(oracle, A, Jy, x, l, u, K.LAMBDA, dtype)
        assert so == M.BoxQPStatus.numericError, what
        res = K.run(cell, A, Jy, x, l, u)
        rec = res["rec"][0]
        assert rec["qp_status"] == so, (what, rec)
        assert rec["lambda"] == np.dtype(dtype).type(K.LAMBDA)
        if not K.writes_on_failure(cell):
            assert K.untouched(res["dx"]) and K.untouched(res["trial"]), what
            assert rec["new_dx_dot"] == 0 and rec["predicted"] == 0 and rec["trial_xnorm"] == 0 and rec["flags"] == 0


# ---------------------------------------------------------------- 7: BOUNDED forced against the automatic class
@pytest.mark.parametrize("cell", FORCED)
def test_forced_bounded_agrees_with_the_automatic_class(oracle, cell):
    auto = cell._replace(box="free")
    if K.cell_class(cell)[1] == "big":                      # one instance a type: the two cells run the same kernel
        assert K.cell_class(auto) == K.cell_class(cell)
    else:
        assert K.cell_class(auto)[3] is False and K.cell_class(cell)[3] is True
    for name in K.POINTS:
        r = K.reference(oracle, cell.n, cell.dtype, cell.box, name)
        tol = B.x_tolerance(cell.dtype, r["P"], r["ora64"][1], r["ora"][1])
        for k, (a, b) in enumerate(zip(launches(oracle, cell, name), launches(oracle, auto, name))):
            ra, rb = a["rec"][0], b["rec"][0]
            assert (ra["qp_status"], ra["flags"], ra["qp_iterations"]) == (rb["qp_status"], rb["flags"], rb["qp_iterations"]), (name, k)
            if ra["qp_status"] == 0:
                assert np.max(np.abs(a["dx"][0].astype(np.float64) - b["dx"][0].astype(np.float64))) <= tol[k], (name, k)


# ---------------------------------------------------------------- every listed class runs
def test_every_listed_class_is_reported_as_run(oracle):
    seen = {}
    for c in K.CELLS:
        key = K.cell_class(c)
        if key in seen:
            continue
        r = K.reference(oracle, c.n, c.dtype, c.box, "zero")
        res = K.run(c, r["JJ"][0], r["Jy"][0], r["x"][0], r["l"][0], r["u"][0])
        seen[(np.dtype(c.dtype).itemsize,) + res["cls"]] = c
    assert set(seen) == {k for k, s in K.LISTED.items() if s == "run"}
    big = [c for c in K.CELLS if c.n > 256]
    for c in big[:1] + [c for c in big if c.one_workgroup][:1]:
        r = K.reference(oracle, c.n, c.dtype, c.box, "zero")
        res = K.run(c, r["JJ"][0], r["Jy"][0], r["x"][0], r["l"][0], r["u"][0])
        assert (res["helpers"] == 1) == c.one_workgroup
    for key in sorted(WORST, key=str):
        print(key, {k: round(v, 4) for k, v in sorted(WORST[key].items())})
