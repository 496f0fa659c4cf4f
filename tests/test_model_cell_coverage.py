"""CPU tier of the model-residual cells (tests/model_cases.py, run on the device by tests/test_gpu_model_cells.py and
tests/test_gpu_tanh_cells.py): the cells reach every instantiated kernel -- through the library's own class function, which is
host code -- and nothing unlisted; the class function is the by-hand restatement over n = 1..513 and the p, m and alignment axes;
the exact data is exact and has the shares the method asks for; the derived bounds hold for a numpy restatement in three summation
orders; and every planted mistake fails the assertion meant for it, by name."""
import fractions

import numpy as np
import pytest

from mir_optim_amd import workloads as W
import model_cases as MC


def test_long_double_has_at_least_63_mantissa_bits():
    assert np.finfo(np.longdouble).nmant >= 63


def test_tanh_inputs_cross_every_rounding_boundary_of_the_exponent_index():
    mag = MC.tanh_magnitudes()
    assert mag[0] == 0 and mag[1] == 5e-324 and np.isinf(mag[-1]) and (mag == 1e300).any() and mag.size > 200000
    assert np.all(np.isin(np.ldexp(1.0, -np.arange(1, 1075)), mag))
    for k in range(58):                                        # (k = 58's boundary lies behind the clamp at 2 |x| = 40)
        v = MC.neighbours(MC.rint_boundary(k))
        idx = np.rint(np.minimum(2.0 * v, 40.0) * MC.LOG2E)
        assert set(idx.tolist()) == {float(k), float(k + 1)}, k
        assert np.all(np.isin(v, mag))
    v = MC.neighbours(20.0)
    assert (2 * v < 40).sum() == 8 and (2 * v > 40).sum() == 8


# ------------------------------------------------------------------------------------------------------------ coverage
def test_cells_reach_every_instance_and_nothing_unlisted():
    seen, paths = set(), set()
    for c in MC.all_tanh_cells():
        args = MC.cell_class_args(c)
        cls = W.tanh_linear_class(**args)
        inst = MC.instances_of(cls, c.dtype)
        base = c.op == "fbd" and c.p == 2 * c.n + 1
        if base and "BASE" not in cls.flags:                   # the extra point's own sweep
            assert cls.launches == 2
            inst |= MC.instances_of(W.tanh_linear_class("f", c.m, c.n, a_A=args["a_A"]))
        assert inst <= MC.INSTANCES, (c, inst - MC.INSTANCES)
        seen |= inst
        if MC.dma_path(cls, c.dense):
            paths.add(MC.dma_path(cls, c.dense))
    assert seen == MC.INSTANCES, sorted(MC.INSTANCES - seen)
    assert paths == MC.DMA_PATHS, sorted(MC.DMA_PATHS ^ paths)
    assert len(MC.INSTANCES) == 2 * 2 * (1 + 8) + 3 + 4 + 13 + 3 + 2


def test_fall_through_cells_land_where_the_class_function_says():
    fb = {(c.n, c.p, c.sA, c.sX): W.tanh_linear_class(**MC.cell_class_args(c)).family for c in MC.fb_cells()["multi"]}
    assert fb[(32, 8, 0, 0)] == "MULTI" and fb[(32, 9, 0, 0)] == "DMA" and fb[(34, 9, 0, 0)] == "MFMA" and fb[(2, 9, 0, 0)] == "LOOP"
    assert fb[(33, 2, 0, 0)] == "LOOP" and fb[(34, 2, 1, 0)] == "MFMA" and fb[(64, 2, 0, 1)] == "DMA" and fb[(2, 2, 1, 0)] == "LOOP"
    n = 64
    assert W.tanh_linear_class("fbd", 65, n, 2 * n, read_a_once=True).mode == 1
    assert W.tanh_linear_class("fbd", 65, n, 2 * n + 16, read_a_once=True).mode == 0       # back to the chunked sweep
    assert W.tanh_linear_class("fbd", 65, 256, 512, read_a_once=True).mode == 0            # not offered at n = 256
    assert W.tanh_linear_class("fbd", 65, 128, 257) == ("DMA", 32, frozenset(["RM", "DIFF", "BASE"]), 2, 1)
    assert W.tanh_linear_class("fbd", 65, 128, 257, dense=True) == ("DMA", 32, frozenset(["RM", "DIFF", "BASE"]), 0, 1)
    assert W.tanh_linear_class("fbd", 65, 128, 257, read_a_once=True) == ("DMA", 32, frozenset(["RM", "DIFF"]), 1, 2)
    assert W.tanh_linear_class("fbd", 65, 64, 129).launches == 2


@pytest.mark.parametrize("op", ["f", "g", "fb", "fbr", "fbd"])
def test_class_function_is_the_restatement_by_hand(op):
    count = 0
    for n in range(1, 514):
        ps = (1,) if op in ("f", "g") else (0, 1, 2, 7, 8, 9, 15, 16, 17, 32, 2 * n - 2, 2 * n, 2 * n + 1, 2 * n + 16)
        for p in ps:
            for m in (0, 1, 31, 32, 33, 64):
                for a_A, a_x, a_y in ((0, 0, 0), (8, 0, 0), (0, 8, 0), (0, 0, 8)):
                    for once, dense in ((False, False), (True, False), (False, True)) if op == "fbd" else ((False, False),):
                        kw = dict(op=op, m=m, n=n, p=p, a_A=a_A, a_x=a_x, a_y=a_y, read_a_once=once, dense=dense)
                        assert tuple(W.tanh_linear_class(**kw)) == MC.hand_class(**kw), kw
                        count += 1
        if op in ("f", "g"):
            for a_A in (0, 4, 8, 12):
                kw = dict(op=op, m=5, n=n, a_A=a_A, elem=4)
                assert tuple(W.tanh_linear_class(**kw)) == MC.hand_class(**kw), kw
    assert count > 500
    with pytest.raises(ValueError):
        W.tanh_linear_class("fb", 5, 5, 5, elem=4)


def test_gauss_sum_class():
    for K in MC.GAUSS_K:
        n = 3 * K + 1
        regs = K <= MC.KGAUSSMAX
        for m in MC.GAUSS_M:
            assert W.gauss_sum_class("f", m, n) == ("k_gauss_sum", regs)
            assert W.gauss_sum_class("fb", m, n, 7) == ("batched_pm", False)
            for p in (0, 1, 7, 32, 100):
                blocks = MC.gauss_blocks(m * p)
                fixed = regs and p > 0 and (blocks * 256) % p == 0
                assert W.gauss_sum_class("fbr", m, n, p) == ("batched_rm", fixed), (K, m, p)
    # both instances of the row-major kernel, both branches of k_gauss_sum, are reached by test_gauss_sum's p = 7, 32 and K = 16, 17
    assert W.gauss_sum_class("fbr", 257, 16, 32)[1] and not W.gauss_sum_class("fbr", 257, 16, 7)[1] and not W.gauss_sum_class("fbr", 257, 52, 32)[1]
    with pytest.raises(ValueError):
        W.gauss_sum_class("g", 5, 16)


# ------------------------------------------------------------------------------------------------------------ the data
def test_exact_cells_are_exact_and_have_the_shares():
    done = set()
    for c in MC.all_tanh_cells():
        key = (c.m, c.n, c.p, c.points, np.dtype(c.dtype).name)
        if key in done or c.m * c.n * c.p > 600_000:           # (the large cells share their generator with the small ones)
            continue
        done.add(key)
        exact, saturated, small = MC.exact_conditions(MC.cell_data(c))
        assert exact, c
        assert saturated <= 0.02, (c, saturated)
        if c.m * c.p >= 64:                                    # (a share of a handful of sums is no share)
            assert small >= 0.25, (c, small)
    assert len(done) > 300


def test_scale_of_the_exact_data():
    for n in (1, 2, 7, 32, 33, 128, 256, 512):
        d = MC.exact_data(512, n, 64)
        s = MC.sums(d)
        body = np.delete(s, [512 // 2, 512 // 3], axis=0)
        assert 0.6 <= body.std() <= 1.9, (n, body.std())
        assert (np.abs(s[512 // 2]) >= 19.06).any() or n == 1
        assert not s[512 // 3].any()
        X2 = d.X.copy()
        X2[:, [0, n - 1]] = X2[:, [n - 1, 0]]
        if n > 1:
            assert np.mean((d.A @ X2.T) != s) > 0.75, n         # swapping two columns of X moves most sums


# ------------------------------------------------------------------------------------------------------------ the bounds
def test_real_bound_holds_for_a_restatement_in_three_orders():
    T = np.tanh                                                # libm's tanh: inside E_T of the long-double one
    for op, m, n, p, base in (("fb", 33, 34, 9, False), ("fbr", 17, 128, 17, False), ("fbd", 33, 64, 128, False), ("fbd", 9, 33, 67, True),
                              ("f", 65, 257, 1, False)):
        for scale in (1.0, 8.0):
            d = MC.real_data(m, n, p - base, scale=scale, base=base)
            ref, bound = MC.real_reference(d, op, base)
            for order in ("forward", "backward", "pairs"):
                r = MC.check_real(MC.restated(d, op, T, base, order=order), ref, bound)
                assert 0 < r <= 1.0
    assert MC.E_T <= 2.0 ** -51


def test_exact_reference_does_not_feel_the_summation_order():
    c = MC.cell("fbd", 33, 128, 257, points="fd")
    d = MC.cell_data(c)
    want = MC.layout(MC.residuals(np.tanh(MC.sums(d)), d.b), "fbd", base=True)
    for order in ("forward", "backward", "pairs"):
        MC.check_band(MC.guarded(MC.restated(d, "fbd", np.tanh, True, order=order)), want, want.size)


# ------------------------------------------------------------------------------------------------------------ planted mistakes
def _fails(name, fn):
    with pytest.raises(AssertionError) as e:
        fn()
    assert str(e.value).startswith(name), (name, str(e.value)[:200])


def test_planted_mistakes_fail_by_name():
    T = np.tanh
    d = MC.cell_data(MC.cell("fb", 33, 34, 9))
    want = {op: MC.layout(MC.residuals(T(MC.sums(d)), d.b), op) for op in ("fb", "fbr")}
    MC.check_band(MC.guarded(MC.restated(d, "fb", T)), want["fb"], want["fb"].size)
    # rows and points transposed in a store; the last column pair dropped; a K permutation applied to A but not to X; b of the wrong row
    for mistake in ("transposed-store", "last-pair-dropped", "k-permutation-on-A-only", "b-of-wrong-row"):
        for op in ("fb", "fbr"):
            _fails("values", lambda: MC.check_band(MC.guarded(MC.restated(d, op, T, mistake=mistake)), want[op], want[op].size))
    # the pair difference with its sign reversed; the base point's residual taken from point 2n - 1
    db = MC.cell_data(MC.cell("fbd", 33, 64, 129, points="fd"))
    wb = MC.layout(MC.residuals(T(MC.sums(db)), db.b), "fbd", base=True)
    MC.check_band(MC.guarded(MC.restated(db, "fbd", T, True)), wb, wb.size)
    for mistake in ("pair-sign-reversed", "base-from-point-2n-1"):
        _fails("values", lambda: MC.check_band(MC.guarded(MC.restated(db, "fbd", T, True, mistake=mistake)), wb, wb.size))
    # a clamped duplicate point stored past p (point-major: behind the last point); a partial stage's last row stored (row-major: row m)
    for op, extra in (("fb", 33), ("fbr", 9)):
        g = MC.guarded(want[op])
        g[MC.GUARD + want[op].size:MC.GUARD + want[op].size + min(extra, MC.GUARD)] = 0.5
        _fails("back-guard", lambda: MC.check_band(g, want[op], want[op].size))
    g = MC.guarded(want["fb"])
    g[MC.GUARD - 1] = 0.5                                       # Y shifted by one element and the aligned pair store kept
    _fails("front-guard", lambda: MC.check_band(g, want["fb"], want["fb"].size))
    # in the point-major layout row m of a point is the next point's row 0
    wrong = want["fb"].copy()
    wrong[33] = 0.5
    _fails("values", lambda: MC.check_band(MC.guarded(wrong), want["fb"], want["fb"].size))
    # the Jacobian's 1 - t t rounded one way for some rows and the other way for the rest
    t = T(MC.sums(d))[:, 0]
    sep, fused = MC.jacobian_candidates(t, d.A)
    if not MC.same_bits(sep, fused):
        mixed = np.where(np.arange(sep.size) < sep.size // 2, sep, fused)
        if not (MC.same_bits(mixed, sep) or MC.same_bits(mixed, fused)):
            _fails("values", lambda: MC.check_band(MC.guarded(mixed), [sep, fused], sep.size))
    # a NaN mapped to 1
    dn = MC.cell_data(MC.cell("fbr", 33, 33, 9))
    dn.X[4, 7] = np.nan
    with np.errstate(invalid="ignore"):
        y = MC.restated(dn, "fbr", T, mistake="nan-to-one").reshape(33, 9)
        assert np.isnan(MC.restated(dn, "fbr", T).reshape(33, 9)[:, 4]).all()
    with pytest.raises(AssertionError, match="nan-to-one"):
        assert np.all(np.isnan(y[:, 4])), "nan-to-one: the outputs a NaN feeds are numbers"
    # the real-valued bound: one ulp-scale slip of the sum passes, a slip of 1e-13 does not
    dr = MC.real_data(33, 34, 9)
    ref, bound = MC.real_reference(dr, "fbr")
    _fails("real-bound", lambda: MC.check_real(MC.restated(dr, "fbr", T) + 1e-13, ref, bound))


def test_gauss_reference_catches_a_sign_and_an_order():
    K, m = 5, 33
    t, data, X = MC.gauss_inputs(m, K, 3)
    x = X[0]
    E = np.exp(MC.gauss_arguments(t, x, K))
    want = MC.gauss_reference(t, data, x, K, E)
    with np.errstate(over="ignore"):
        nosign = np.exp(-MC.gauss_arguments(t, x, K))           # gauss_g without its sign
    _fails("values", lambda: MC.check_band(MC.guarded(MC.gauss_reference(t, data, x, K, nosign)), want, m))
    plain = x[3 * K] + (x[None, :K] * E).sum(axis=1) - data     # unfused, another order: close, and not the bits
    assert np.allclose(plain, want, rtol=0, atol=1e-14) and not MC.same_bits(plain, want)
    assert np.all(MC.gauss_arguments(t, X[-1], K)[:, 0] < -5e5)  # the tiny width underflows for every row
    # the float rounding of the exact fused multiply-add: against numpy's own double arithmetic where that is exact
    rng = np.random.default_rng(1)
    for _ in range(2000):
        a, b, c = rng.standard_normal(3).astype(np.float32)
        fr = MC.round_fraction(fractions.Fraction(float(a)) * fractions.Fraction(float(b)), np.float32)
        assert fr == np.float32(np.float64(a) * np.float64(b))  # a product of floats is exact in double: one rounding
        assert MC.fma_exact(a, b, np.float32(0), np.float32) == fr
