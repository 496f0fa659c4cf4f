"""CPU tier of the read-only Broyden sweep's kernel-level tests (tests/lr_cases.py, run on the device by tests/test_gpu_lr_cells.py):
the cells reach every instantiated instance of the sweep and the flush through the library's own class function (mir_lsq_lr_class,
host code) and nothing else, and name what the axes say; the exact-integer generators are exact, inside their magnitude bound, for
every cell; the numpy restatement of a pass stays inside the derived bounds in three summation orders; and each planted mistake in
that restatement fails the assertion meant to catch it."""
import numpy as np
import pytest

from mir_optim_amd import api
import lr_cases as K

DT = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


def test_cells_cover_exactly_the_instantiated_instances():
    image = {}
    for c in K.CELLS:
        for key in K.cell_classes(c):
            image.setdefault(key, []).append(c)
    assert len(K.LISTED) == 40
    assert set(image) - K.LISTED == set(), "cells on instances the list does not have"
    assert K.LISTED - set(image) == set(), "listed instances no cell reaches"
    for (es, kern, ncp, vec), cells in image.items():       # the non-vector instances through an odd n AND a shifted even n
        if not vec:
            assert {(c.n % 2, c.off) for c in cells if c.kind != "chain"} >= {(1, 0), (0, 1)}, (es, kern, ncp)


def test_the_class_function_against_a_table_written_by_hand():
    for es in (4, 8):
        for n in range(1, 513):
            ncp = 1 if n <= 32 else 2 if n <= 64 else 4 if n <= 128 else 8 if n <= 256 else 16
            for aligned in (False, True):
                assert api.lr_class(es, n, aligned) == (ncp, aligned and n % 2 == 0), (es, n, aligned)
    for bad in ((2, 8), (8, 0), (8, 513)):
        with pytest.raises(ValueError):
            api.lr_class(*bad)


def test_the_workgroup_count_and_the_row_axis():
    for num_cu in (1, 64, 256, 304):
        for m in (1, 3, 4, 5, 127, 128, 129, K.M_N, K.M_RAGGED, K.M_REDUCE, K.M_GRID, 10 ** 7):
            assert api.lr_blocks(m, num_cu) == K.blocks_by_hand(m, num_cu), (m, num_cu)
    cu = 256
    assert [api.lr_blocks(m, cu) for m in (127, 128, 129)] == [1, 1, 2]
    assert api.lr_blocks(K.M_REDUCE, cu) == 34 > 32                      # k_lr_reduce / lr_reduce_scalar past 32 ranges, 15 of them empty
    assert api.lr_blocks(K.M_GRID, cu) == api.LR_MAX_BLOCKS and api.lr_blocks(K.M_GRID - 200, cu) < api.LR_MAX_BLOCKS and K.M_GRID > 131072
    for m in (K.M_N, K.M_RAGGED):                                        # a trip's spare slots re-read the last group (unroll 4 and 2)
        per = K.groups_per_wave(m, api.lr_blocks(m, cu))
        assert per % 4 != 0 and per % 2 != 0 and api.lr_blocks(m, cu) > 1 and m % 4 != 0, (m, per)


def test_cell_list_is_what_the_issue_names():
    for dt in K.DTYPES:
        mine = [c for c in K.CELLS if c.dtype == dt]
        for kind in ("pass", "flush"):
            assert {c.n for c in mine if c.kind == kind and c.m == K.M_N and c.off == 0} >= set(K.NS)
            assert {c.n for c in mine if c.kind == kind and c.off == 1} == {n for n in K.NS if n % 2 == 0}
            assert {c.m for c in mine if c.kind == kind} >= {1, 3, 4, 5, 127, 128, 129, K.M_RAGGED, K.M_REDUCE, K.M_GRID}
        assert {c.k for c in mine if c.kind == "pass" and c.mode == "plain"} >= {0, 1, 4, 5, 15}
        assert {c.k for c in mine if c.kind == "flush"} >= {1, 2, 15, 16}
        assert any(c.kind == "flush" and (c.k, c.n) == (16, 512) for c in mine)
        assert {c.mode for c in mine if c.kind == "pass"} == {"plain"} | set(K.GO) | set(K.NOGO)
        assert {c.count for c in mine if c.kind == "pass"} == {1, K.COUNT_MAX} and K.COUNT_MAX == 8
        assert {c.count for c in mine if c.mode in K.NOGO} == {1, K.COUNT_MAX} == {c.count for c in mine if c.mode in K.GO}
        assert any(c.count > 1 and api.lr_blocks(c.m, 256) > 32 for c in mine)
        assert {c.n for c in mine if c.kind == "chain"} == set(K.CHAIN_NS)
        assert {api.lr_class(8, n)[0] for n in K.CHAIN_NS} == {1, 2, 4}
        assert all(c.m <= K.M_REDUCE for c in mine if c.n == 512) and all(c.n <= 8 for c in mine if c.m > 131072)
        es = np.dtype(dt).itemsize                          # no cell allocates more than about 20 MB
        assert max(es * (c.m * c.n + (c.k + 1) * (c.m + c.n) + (c.count + 1) * c.m + c.n * c.n) for c in mine) < 20e6


@pytest.mark.parametrize("dtype", DT)
def test_speculation_records_say_what_they_are_named(dtype):
    for mode in K.GO:
        assert K.spec_go_by_hand(*K.spec_of(mode, dtype))
    for mode in K.NOGO:
        rec, at, rt = K.spec_of(mode, dtype)
        assert not K.spec_go_by_hand(rec, at, rt)
        go = K.spec_of("go", dtype)                          # exactly one thing differs from the go record
        diff = [key for key in rec if rec[key] != go[0][key]] + (["at"] if at != go[1] else []) + (["rt"] if rt != go[2] else [])
        assert len(diff) == 1, (mode, diff)


@pytest.mark.parametrize("dtype", DT)
def test_exact_generators_stay_exact_for_every_cell(dtype):
    seen = set()
    worst = 0.0
    for c in K.CELLS:
        if c.dtype != dtype or c.kind == "chain" or (c.kind, c.m, c.n, c.k) in seen:
            continue
        seen.add((c.kind, c.m, c.n, c.k))
        inp = K.exact_inputs(c.m, c.n, c.k, dtype, max(c.count, 1))
        for key, v in inp.items():
            assert v.dtype == dtype and np.array_equal(v.astype(np.float64), np.rint(v.astype(np.float64))), key
        if c.kind == "pass":
            worst = max(worst, K.assert_exact(inp, K.wide_pass(inp)))
            if c.m * c.n <= 10000:                           # the restatement in the type reproduces the wide values: the data is exact
                res = K.standin_pass(inp)
                K.check_exact_pass(res, inp)
                K.check_bits(res, inp)
        else:
            ref, ab = K.wide_flush(inp)
            K.check_exact_flush(ref.astype(dtype), inp)
            worst = max(worst, float(ab.max()))
    print(f"{np.dtype(dtype).name}: largest sum of absolute values {worst:.0f} of {K.EXACT_LIMIT:.0f}")


RESTATED = [(K.M_N, 35, 5), (K.M_N, 36, 0), (5, 7, 4), (K.M_RAGGED, 40, 15), (1, 1, 1), (K.M_N, 130, 5)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("m,n,k", RESTATED)
def test_restatement_stays_inside_the_bounds_in_three_orders(m, n, k, dtype):
    inp = K.random_inputs(m, n, k, dtype)
    worst = {}
    for order in (0, 1, 2):
        res = K.standin_pass(inp, order)
        for key, v in zip(("u", "reduced", "JJ", "Jy"), (K.check_u(res, inp), K.check_reduced(res, inp)) + K.check_finish(res, inp)):
            worst[key] = max(worst.get(key, 0.0), v)
        K.check_bits(res, inp)
        K.check_sums(res, inp)
    print(f"m = {m} n = {n} k = {k} {np.dtype(dtype).name}: largest error / bound of the restatement", {a: round(v, 4) for a, v in worst.items()})
    fin = dict(J=inp["J"], U=inp["U"], D=inp["D"])
    if k:
        Jf = inp["J"].copy()
        for l in range(k):
            Jf = Jf + np.outer(inp["U"][l], inp["D"][l])
        assert K.check_flush(Jf, fin) <= 1
        with pytest.raises(AssertionError, match="^flush:"):
            K.check_flush(Jf - np.outer(inp["U"][k - 1], inp["D"][k - 1]), fin)


# the planted mistake and the assertion meant to catch it
PLANTED = [("drop_last_rows", "reduced"), ("spare_row_twice", "reduced"), ("skip_pending", "u"), ("coef_next_D", "u"), ("swap_y", "u"),
           ("no_uu", "JJ"), ("no_transpose_partner", "JJ"), ("drop_last_col", "reduced"), ("h_for_w", "Jy")]
PLANTED_SHAPE = (5, 7, 4)    # the smallest cell with a whole row group AND a ragged tail; odd n, k >= 2: every mistake exists on it


def _all_checks(res, inp):
    K.check_u(res, inp)
    K.check_reduced(res, inp)
    K.check_finish(res, inp)
    K.check_bits(res, inp)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("mutate,name", PLANTED)
def test_a_planted_mistake_fails_its_assertion(mutate, name, dtype):
    assert mutate in K.MUTATIONS
    m, n, k = PLANTED_SHAPE
    assert any((c.m, c.n, c.k) == PLANTED_SHAPE and c.kind == "pass" and c.dtype == dtype for c in K.CELLS), "not a cell"
    inp = K.random_inputs(m, n, k, dtype)
    _all_checks(K.standin_pass(inp), inp)
    bad = K.standin_pass(inp, mutate=mutate)
    with pytest.raises(AssertionError, match="^" + name + ":"):
        _all_checks(bad, inp)
    if mutate == "no_transpose_partner":
        with pytest.raises(AssertionError, match="^symmetry:"):
            K.check_bits(bad, inp)
    ex = K.exact_inputs(m, n, k, dtype)                      # ... and the exact-integer check sees it too
    K.check_exact_pass(K.standin_pass(ex), ex)
    with pytest.raises(AssertionError, match="^exact:"):
        K.check_exact_pass(K.standin_pass(ex, mutate=mutate), ex)


def test_every_planted_mistake_is_listed():
    assert {p[0] for p in PLANTED} == set(K.MUTATIONS)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", K.CHAIN_NS)
def test_the_chain_identity_holds_for_the_restatement(n, dtype):
    def flush(cell, fin):
        Jf = fin["J"].copy()
        for l in range(fin["U"].shape[0]):
            Jf = Jf + np.outer(fin["U"][l], fin["D"][l])
        return Jf
    ratios = K.chain(K.Cell("chain", dtype, K.M_N, n, 0, 0, "", 0), lambda c, inp: K.standin_pass(inp), flush)
    print(f"n = {n} {np.dtype(dtype).name}: error / bound of JJ, Jy, the flushed J", [round(r, 4) for r in ratios])
    assert all(r <= 1 for r in ratios)
