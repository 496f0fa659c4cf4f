"""CPU tier of the LM solve launch tests (tests/lm_solve_cases.py, run on the device by tests/test_gpu_lm_solve.py): the cells reach
every instantiated kernel class through the library's own dispatch (mir_lsq_lm_solve_class, host code) with both parities of n
wherever the J^T J copy loop runs; the margin screen drops at most SINGLE_MAX_SCREENED_OUT of a family's 16 problems; the numpy
restatement of the epilogue stays inside the first-order bounds in three summation orders; and each planted mistake in that
restatement fails the assertion named for it."""
import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api
import boxqp_cases as B
import lm_solve_cases as K

DT = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
RESTATED_NS = (1, 2, 7, 16, 33, 129, 300)


def _as_result(epilogue, dtype):
    """standin_epilogue's tuple in the shape of a launch's result (one ladder entry)"""
    d, tr, ndd, pred, xn, flags = epilogue
    rec = np.zeros(1, dtype=api.lm_solve_record_dtype(dtype))
    rec["new_dx_dot"], rec["predicted"], rec["trial_xnorm"], rec["flags"] = ndd, pred, xn, flags
    return {"rec": rec, "dx": d[None, :], "trial": tr[None, :]}


def test_cells_cover_exactly_the_listed_classes():
    image = {}
    for c in K.CELLS:
        image.setdefault(K.cell_class(c), []).append(c)
    run = {k for k, s in K.LISTED.items() if s == "run"}
    assert set(image) - run == set(), "cells on classes the list does not have (or must not run)"
    assert run - set(image) == set(), "listed classes no cell reaches"
    assert {k for k, s in K.LISTED.items() if s != "run"} == {(8, "workgroup", 1, False), (8, "workgroup", 1, True)}
    for b in (False, True):                                  # ... which the diagnostic buffer reaches, and nothing else
        assert api.lm_solve_class(8, 16, b, diagnostic=True) == ("workgroup", 1, b)
    assert len(K.LISTED) == 2 + 10 + 10 + 2
    for key, cells in image.items():
        if K.has_copy_loop(key):
            assert {c.n % 2 for c in cells} == {0, 1}, (key, sorted(c.n for c in cells))
    assert len(set(K.CELLS)) == len(K.CELLS)


def test_the_dispatch_against_a_table_written_by_hand():
    def by_hand(es, n, bounded, generic):
        if generic or n > 256:
            return ("big", 0, True)
        if es == 8 and n <= 16:
            return ("wave", 0, bounded)
        return ("workgroup", 1 if n <= 16 else 2 if n <= 32 else 4 if n <= 64 else 8 if n <= 128 else 0, bounded)
    for es in (4, 8):
        for n in list(range(1, 300)) + [1000, 4096]:
            for bounded in (False, True):
                for generic in (False, True):
                    assert api.lm_solve_class(es, n, bounded, generic) == by_hand(es, n, bounded, generic), (es, n, bounded, generic)
    with pytest.raises(ValueError):
        api.lm_solve_class(2, 8, True)


def test_cell_list_is_what_the_issue_names():
    ns = {dt: {c.n for c in K.CELLS if c.dtype == dt and not c.generic and not c.one_workgroup} for dt in K.DTYPES}
    assert ns[np.float32] == set(K.NS) and ns[np.float64] == set(K.NS) | {7, 9}
    for dt in K.DTYPES:
        for n in ns[dt]:
            assert {c.box for c in K.CELLS if (c.n, c.dtype, c.generic, c.one_workgroup) == (n, dt, False, False)} == set(K.BOXES)
        assert {c.n for c in K.CELLS if c.dtype == dt and c.generic} == {16, 100}
        assert {c.n for c in K.CELLS if c.dtype == dt and c.one_workgroup} == {257, 300}
    assert K.LADDER[0] == K.LAMBDA and all(b / a == 10 * 2 ** k for k, (a, b) in enumerate(zip(K.LADDER, K.LADDER[1:])))
    assert np.isfinite(np.float32(K.LADDER[-1]))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", K.NS + K.NS_F64_EXTRA)
def test_margin_screen_drops_few_problems(oracle, n, dtype):
    """x = 0, the family's box, lambda = 1 / 8: every problem solved by both oracles, at most 2 of 16 inside the margin"""
    r = K.reference(oracle, n, dtype, "box", "zero")
    assert np.all(r["ora"][0] == 0) and np.all(r["ora64"][0] == 0)
    out = int(np.count_nonzero(~r["screened"]))
    print(f"n = {n} {np.dtype(dtype).name}: {out} of {K.COUNT} screened out")
    assert out <= B.SINGLE_MAX_SCREENED_OUT
    scr = r["screened"]
    assert np.array_equal(r["ora"][2][scr], r["ora64"][2][scr])
    free = K.reference(oracle, n, dtype, "free", "zero")
    assert np.all(free["screened"]) and np.all(free["ora"][2] == 0)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", RESTATED_NS)
def test_restatement_stays_inside_the_bounds_in_three_orders(oracle, n, dtype):
    worst = {}
    for box in ("free", "box"):
        for name in K.POINTS:
            if not K.point_problems(name, box):
                continue
            r = K.reference(oracle, n, dtype, box, name)
            for k in range(min(len(r["idx"]), 2)):
                xq = r["ora"][1][k]
                for order in (0, 1, 2):
                    res = _as_result(K.standin_epilogue(xq, r["JJ"][k], r["Jy"][k], r["x"][k], r["l"][k], r["u"][k], K.LAMBDA, dtype,
                                                        np.inf, order), dtype)
                    ratios = K.check_epilogue(res, 0, r["JJ"][k], r["Jy"][k], r["x"][k], r["l"][k], r["u"][k], dtype, np.inf)
                    for key, v in ratios.items():
                        worst[key] = max(worst.get(key, 0.0), v)
                    if name in ("zero", "inside", "null"):
                        assert bool(res["rec"][0]["flags"] & api.LM_FLAG_NULL_STEP) == (name == "null")
                    if name == "huge_some":                   # the rounding zeroes the steps of the huge coordinates, or leaves
                        S = np.arange(n) % 3 == 0             # a multiple of their spacing
                        assert np.all(res["dx"][0][S] % np.spacing(dtype(K.HUGE[dtype])) == 0) and np.any(res["dx"][0][S] == 0)
    print(f"n = {n} {np.dtype(dtype).name}: largest error / bound of the restatement", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1 for v in worst.values())


def _mutation_case(n, dtype):
    """a problem on which every planted mistake shows: the family's, free, at the point with huge coordinates (the rounding of
    the step matters) -- and for the clamp a point below its box"""
    P, q, l, u = K.problem(n, dtype, "free", 0)
    x, l, u = K.point("huge_some", n, dtype, "free", 0)
    return P, q, x, l, u


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("mutate,name", [("damped", "predicted"), ("no_diag", "predicted"), ("unclamped", "trial"),
                                         ("unrounded_ndd", "new_dx_dot")])
def test_a_planted_mistake_in_the_epilogue_fails_its_assertion(oracle, dtype, mutate, name):
    n = 33
    JJ, Jy, x, l, u = _mutation_case(n, dtype)
    s = M.LeastSquaresSettings(dtype)
    if mutate == "unclamped":
        # the QP keeps its solution inside the shifted box, so the clamp only ever undoes a rounding: the epilogue is handed a
        # step that leaves the box by one unit in every third coordinate instead
        u = np.where(np.arange(n) % 3 == 1, x + 0.5, u)
        xq = np.where(np.arange(n) % 3 == 1, 1.5, 0.25)
        res = [_as_result(K.standin_epilogue(xq, JJ, Jy, x, l, u, K.LAMBDA, dtype, s.maxStep, 0, m), dtype) for m in (None, mutate)]
        K.check_epilogue(res[0], 0, JJ, Jy, x, l, u, dtype, s.maxStep)
        with pytest.raises(AssertionError, match="^" + name + ":"):
            K.check_epilogue(res[1], 0, JJ, Jy, x, l, u, dtype, s.maxStep)
        return
    good = K.standin_launch(oracle, JJ, Jy, x, l, u, (K.LAMBDA,), dtype, s)
    assert good["rec"][0]["qp_status"] == 0
    K.check_epilogue(good, 0, JJ, Jy, x, l, u, dtype, s.maxStep)
    bad = K.standin_launch(oracle, JJ, Jy, x, l, u, (K.LAMBDA,), dtype, s, mutate=mutate)
    with pytest.raises(AssertionError, match="^" + name + ":"):
        K.check_epilogue(bad, 0, JJ, Jy, x, l, u, dtype, s.maxStep)


@pytest.mark.parametrize("dtype", DT)
def test_a_planted_mistake_in_lambda0_fails_its_assertion(oracle, dtype):
    n = 33
    JJ, Jy, x, l, u = _mutation_case(n, dtype)
    JJ = K.lambda0_tie(JJ)
    d = JJ[-1, -1]
    assert JJ[0, 0] == -d and np.abs(np.diagonal(JJ)[1:-1]).max() == d / 2
    s = M.LeastSquaresSettings(dtype)
    good = K.standin_launch(oracle, JJ, Jy, x, l, u, (K.LAMBDA,), dtype, s, lambda_from_state=True)
    assert good["rec"][0]["lambda"] == 1
    K.check_lambda0(good, JJ, 0.0, s, dtype)
    bad = K.standin_launch(oracle, JJ, Jy, x, l, u, (K.LAMBDA,), dtype, s, lambda_from_state=True, mutate="lambda0_last")
    assert bad["rec"][0]["lambda"] == np.dtype(dtype).type(0.001) * np.dtype(dtype).type(d)
    with pytest.raises(AssertionError, match="^lambda0:"):
        K.check_lambda0(bad, JJ, 0.0, s, dtype)


@pytest.mark.parametrize("dtype", DT)
def test_a_planted_mistake_in_the_ladder_fails_its_assertion(oracle, dtype):
    n = 17
    JJ, Jy, _, _, _ = _mutation_case(n, dtype)
    x, l, u = K.point("inside", n, dtype, "box", 0)
    s = M.LeastSquaresSettings(dtype)
    singles = [K.standin_launch(oracle, JJ, Jy, x, l, u, (lam,), dtype, s) for lam in K.LADDER]
    K.check_ladder(K.standin_launch(oracle, JJ, Jy, x, l, u, K.LADDER, dtype, s), singles)
    with pytest.raises(AssertionError, match="^ladder:"):
        K.check_ladder(K.standin_launch(oracle, JJ, Jy, x, l, u, K.LADDER, dtype, s, mutate="ladder_prev"), singles)


@pytest.mark.parametrize("dtype", DT)
def test_the_gradient_test_of_the_restatement(oracle, dtype):
    n = 9
    JJ, Jy, x, l, u = _mutation_case(n, dtype)
    T = np.dtype(dtype).type
    g = np.abs(Jy.astype(dtype)).max()
    for tol, small in ((g, True), (np.nextafter(g, T(np.inf)), True), (np.nextafter(g, T(0)), False)):
        s = M.LeastSquaresSettings(dtype)
        s.gradTolerance = float(tol)
        res = K.standin_launch(oracle, JJ, Jy, x, l, u, (K.LAMBDA,), dtype, s, check_grad=True)
        assert K.check_gradient(res, Jy, s.gradTolerance, dtype) == small
    s.gradTolerance = float(g)
    res = K.standin_launch(oracle, JJ, Jy, x, l, u, (K.LAMBDA,), dtype, s, check_grad=True)
    res["rec"]["lambda"][0] = K.LAMBDA                          # a record that keeps a field beside the flag fails
    with pytest.raises(AssertionError, match="^gradient:"):
        K.check_gradient(res, Jy, s.gradTolerance, dtype)


def test_points_are_what_they_say():
    for dtype in K.DTYPES:
        for n in (1, 2, 16, 33):
            for p in range(K.FEW):
                x, l, u = K.point("inside", n, dtype, "box", p)
                assert np.all(l <= x) and np.all(x <= u) and np.array_equal(x, x.astype(dtype).astype(np.float64))
                x, l, u = K.point("huge_some", n, dtype, "box", p)
                S = np.arange(n) % 3 == 0
                assert np.all(np.abs(x[S]) == np.float64(dtype(K.HUGE[dtype]))) and np.all(np.isinf(l[S]) & np.isinf(u[S]))
                assert np.all(l <= x) and np.all(x <= u)
                x, l, u = K.point("huge_all", n, dtype, "free", p)
                assert np.all(np.abs(x) == np.float64(dtype(K.HUGE[dtype]))) and {np.sign(v) for v in x} <= {1.0, -1.0}
    assert K.point_problems("zero", "box") == tuple(range(16)) and K.point_problems("huge_all", "box") == K.point_problems("null", "box") == ()
