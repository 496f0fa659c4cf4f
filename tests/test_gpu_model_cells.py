"""The model-residual kernels of csrc/workloads.hip and csrc/workloads_gemm.hip, one call of a C entry at a time between guard
bands, at the cells of tests/model_cases.py (the method, the data and the bounds are derived there; tests/test_model_cell_coverage.py
proves on the CPU that the cells reach every instantiated kernel). Every cell checks: the class the library names is the class
restated by hand; the output BIT FOR BIT (exact tier) or inside the derived bound (real-valued tier, f64 residual entries on cells
small enough for a long-double GEMM on the host); a canary band in front of and behind the output untouched; a second call
gives the same bits; the inputs unchanged.

Measured on an MI355X: this file and test_gpu_tanh_cells.py, 246 tests, in 28 s, the slowest parameter 1.2 s; real-valued tier
at most 0.50 of its bound, the decay at most 0.98 (profiles/r23/model_cells.txt).

A NaN in X or in A comes out finite (dtanh(NaN) = +-1): the containment cells and the solve that ask for NaN
are expected failures, strictly; what the kernels do with it today is pinned next to them."""
import collections
import ctypes as C

import numpy as np
import pytest

from mir_optim_amd import api, workloads as W
import model_cases as MC

pytestmark = pytest.mark.gpu
NAN_REASON = ("dtanh(NaN) = +-1: fmin drops the NaN; both NaN-keeping clamps cost the forked n = 128 GEMM 12 bytes of scratch "
              "memory (profiles/r23/dtanh_nan_resources.txt), so dtanh stays as it is")
RATIOS = collections.defaultdict(float)      # real-valued tier: largest error / bound per (op, family)
_tables = {}


def device_tanh(s):
    """T(s) from the unary entry on the distinct values of s, cached per type"""
    dt = s.dtype.type
    keys, vals = _tables.get(dt, (np.empty(0, MC.bits(s).dtype), np.empty(0, s.dtype)))
    u = np.unique(MC.bits(s))
    new = u[~np.isin(u, keys)]
    if new.size:
        keys = np.concatenate([keys, new])
        vals = np.concatenate([vals, W.unary("tanh", new.view(s.dtype), dtype=dt)])
        order = np.argsort(keys)
        keys, vals = keys[order], vals[order]
        _tables[dt] = (keys, vals)
    return vals[np.searchsorted(keys, MC.bits(s))].reshape(s.shape)


def shifted(a, shift):
    """a device buffer holding a.ravel() `shift` elements behind its (256-byte aligned) start; (buffer, address)"""
    flat = np.concatenate([np.zeros(shift, a.dtype), a.ravel(), np.zeros(2, a.dtype)])
    buf = api.DeviceBuffer(flat)
    return buf, buf.ptr + shift * a.dtype.itemsize


def out_count(c):
    if c.op == "f":
        return c.m
    if c.op == "g":
        return c.m * c.n
    if c.op == "fbd":
        base = c.p == 2 * c.n + 1
        return c.m * ((c.p - base) // 2) + (c.m if base else 0)
    return c.m * c.p


def entry(c):
    WL = api.workloads_lib()
    suf = "d" if c.dtype == np.float64 else "s"
    if c.op in ("f", "g"):
        return getattr(WL, "wl_tanh_linear_%s_%s" % (c.op, suf))
    return getattr(WL, "wl_tanh_linear_fbd_dense_d" if (c.op == "fbd" and c.dense) else "wl_tanh_linear_%s_d" % c.op)


def run_cell(c, d, calls=2, check_inputs=True):
    """the outputs of `calls` calls of c's entry on Data d, each GUARD + count + GUARD elements (MC.check_band's layout)"""
    dt = np.dtype(c.dtype)
    count = out_count(c)
    stream = api.Stream()
    bA, pA = shifted(d.A, c.sA)
    bX, pX = shifted(d.X, c.sX)
    bb = api.DeviceBuffer(d.b)
    ctx = W._TanhCtx(pA, bb.ptr, stream.handle, int(c.once))
    fill = np.concatenate([np.zeros(c.sY, dt), MC.canary(MC.GUARD, dt, 1), MC.canary(count, dt, 0), MC.canary(MC.GUARD, dt, 2)])
    fn, outs = entry(c), []
    try:
        for _ in range(calls):
            bY = api.DeviceBuffer(fill)
            args = [C.c_void_p(C.addressof(ctx)), C.c_size_t(c.m), C.c_size_t(c.n)] + ([] if c.op in ("f", "g") else [C.c_size_t(c.p)])
            fn(*args, C.c_void_p(pX), C.c_void_p(bY.ptr + (c.sY + MC.GUARD) * dt.itemsize))
            stream.synchronize()
            outs.append(bY.download()[c.sY:])
            bY.free()
        if check_inputs:
            n2 = slice(c.sA, c.sA + d.A.size)
            assert MC.same_bits(bA.download()[n2], d.A.ravel()), "inputs: A changed"
            assert MC.same_bits(bX.download()[c.sX:c.sX + d.X.size], d.X.ravel()), "inputs: X changed"
            assert MC.same_bits(bb.download(), d.b), "inputs: b changed"
    finally:
        for b_ in (bA, bX, bb):
            b_.free()
        stream.close()
    return outs, count


def expected_exact(c, d):
    t = device_tanh(MC.sums(d, c.dtype))
    if c.op == "g":
        return MC.jacobian_candidates(t[:, 0], d.A)
    return MC.layout(MC.residuals(t, d.b), c.op, base=(c.op == "fbd" and c.p == 2 * c.n + 1))


def check_cell(c, real=True):
    args = MC.cell_class_args(c)
    cls = W.tanh_linear_class(**args)
    assert tuple(cls) == MC.hand_class(**args), ("class", c, cls, MC.hand_class(**args))
    d = MC.cell_data(c)
    outs, count = run_cell(c, d, check_inputs=MC.is_small(c))
    try:
        MC.check_band(outs[0], expected_exact(c, d), count)
        assert MC.same_bits(outs[0], outs[1]), "second-call: a second call gives other bits"
    except AssertionError as e:
        raise AssertionError("%s  class %s: %s" % (c, cls, e)) from None
    if real and c.dtype == np.float64 and c.op != "g" and MC.is_small(c) and c.points == "random" and not c.once:
        for kind in ("real", "real8"):
            dr = MC.cell_data(c, kind)
            (got,), count = run_cell(c, dr, calls=1, check_inputs=False)
            ref, bound = MC.real_reference(dr, c.op, base=(c.op == "fbd" and c.p == 2 * c.n + 1))
            try:
                r = MC.check_real(got[MC.GUARD:MC.GUARD + count], ref, bound)
            except AssertionError as e:
                raise AssertionError("%s  class %s %s: %s" % (c, cls, kind, e)) from None
            RATIOS[(c.op, cls.family)] = max(RATIOS[(c.op, cls.family)], r)


# ------------------------------------------------------------------------------------------------------------ the exact + real tiers
POINT = [(op, dt, n) for op in ("f", "g") for dt in (np.float64, np.float32) for n in MC.point_cells(op, dt)]


@pytest.mark.parametrize("op,dtype,n", POINT, ids=["%s-%s-n%d" % (o, np.dtype(t).name, n) for o, t, n in POINT])
def test_one_point_entries(op, dtype, n):
    for c in MC.point_cells(op, dtype)[n]:
        check_cell(c)


def _by_n(groups):
    out = collections.OrderedDict()
    for name, cells in groups.items():
        for c in cells:
            out.setdefault("%s-n%d" % (name, c.n), []).append(c)
    return out


FB, FBR, FBD = _by_n(MC.fb_cells()), _by_n(MC.fbr_cells()), _by_n(MC.fbd_cells())


@pytest.mark.parametrize("group", list(FB))
def test_point_major_entry(group):
    for c in FB[group]:
        check_cell(c)


@pytest.mark.parametrize("group", list(FBR))
def test_row_major_entry(group):
    for c in FBR[group]:
        check_cell(c)


@pytest.mark.parametrize("group", list(FBD))
def test_difference_panel_entry(group):
    for c in FBD[group]:
        check_cell(c)


def test_forked_dense_read_once_and_base_agree_and_the_extra_point_is_the_sweeps():
    """one finite-difference point set through every way the n = 128 panel is computed: the same bits (each is also held to the
    reference above), and the extra point's residual is the one-point sweep's"""
    m, n = 8225, 128
    d = MC.exact_data(m, n, 2 * n, fd=True, base=True)
    panels = {}
    for name, kw in (("forked", {}), ("dense", dict(dense=True)), ("once", dict(once=True))):
        for p in (2 * n, 2 * n + 1):
            c = MC.cell("fbd", m, n, p, points="fd", **kw)
            dd = d if p == 2 * n + 1 else MC.Data(d.A, d.X[:-1], d.b, d.S[:, :-1], d.e)
            (got,), count = run_cell(c, dd, calls=1, check_inputs=False)
            panels[(name, p)] = got[MC.GUARD:MC.GUARD + count]
    first = panels[("forked", 2 * n)]
    for k, v in panels.items():
        assert MC.same_bits(v[:m * n], first), k
    (sweep,), _ = run_cell(MC.cell("f", m, n), MC.Data(d.A, d.X[-1:], d.b, d.S[:, -1:], d.e), calls=1, check_inputs=False)
    for name in ("forked", "dense", "once"):
        assert MC.same_bits(panels[(name, 2 * n + 1)][m * n:], sweep[MC.GUARD:MC.GUARD + m]), name


def test_zzz_error_to_bound_ratios():
    """prints the real-valued tier's largest error / bound per entry and family (profiles/r23/model_cells.txt)"""
    check_cell(MC.cell("fbr", 33, 33, 9))                      # (run alone, the table has this one row)
    for k in sorted(RATIOS):
        print("real-valued tier: %-4s %-13s largest error / bound %.4f" % (k + (RATIOS[k],)))
    assert max(RATIOS.values()) <= 1.0


# ------------------------------------------------------------------------------------------------------------ nothing for nothing
ZERO = [MC.cell("f", 0, 32), MC.cell("g", 0, 33), MC.cell("f", 0, 264), MC.cell("f", 0, 32, dtype=np.float32),
        MC.cell("fbr", 64, 32, 0), MC.cell("fbr", 33, 7, 0), MC.cell("fbr", 0, 32, 5), MC.cell("fbr", 0, 264, 5),
        MC.cell("fbd", 33, 7, 0), MC.cell("fbd", 0, 7, 14), MC.cell("fbd", 64, 32, 0), MC.cell("fb", 0, 33, 3), MC.cell("fb", 0, 32, 3)]


@pytest.mark.parametrize("c", ZERO, ids=lambda c: "%s-m%d-n%d-p%d-%s" % (c.op, c.m, c.n, c.p, np.dtype(c.dtype).name))
def test_nothing_is_written_for_no_rows_or_no_points(c):
    """the entries that accept m = 0 or p = 0 (fb with p = 0 reads a point and the GEMM kernels of fb take m > 0: left out)"""
    rng = np.random.default_rng(0)
    m, p = max(c.m, 1), max(c.p, 1)
    d = MC.Data(rng.standard_normal((m, c.n)).astype(c.dtype), rng.standard_normal((p, c.n)).astype(c.dtype), rng.standard_normal(m).astype(c.dtype), None, None)
    dt = np.dtype(c.dtype)
    stream = api.Stream()
    bufs = [api.DeviceBuffer(v) for v in (d.A, d.X, d.b)]
    ctx = W._TanhCtx(bufs[0].ptr, bufs[2].ptr, stream.handle, 0)
    fill = MC.canary(2 * MC.GUARD + 64, dt, 4)
    bY = api.DeviceBuffer(fill)
    args = [C.c_void_p(C.addressof(ctx)), C.c_size_t(c.m), C.c_size_t(c.n)] + ([] if c.op in ("f", "g") else [C.c_size_t(c.p)])
    entry(c)(*args, C.c_void_p(bufs[1].ptr), C.c_void_p(bY.ptr + MC.GUARD * dt.itemsize))
    stream.synchronize()
    assert MC.same_bits(bY.download(), fill)
    for b_ in bufs + [bY]:
        b_.free()


# ------------------------------------------------------------------------------------------------------------ NaN containment
NAN_CELLS = [MC.cell("f", 65, 32), MC.cell("f", 65, 264), MC.cell("fb", 65, 32, 7), MC.cell("fb", 65, 34, 17), MC.cell("fb", 65, 64, 17),
             MC.cell("fbr", 65, 128, 17), MC.cell("fbd", 65, 128, 256, points="fd"), MC.cell("fbd", 65, 64, 128, dense=True),
             MC.cell("fb", 65, 264, 18), MC.cell("fbr", 33, 33, 9), MC.cell("fbd", 33, 33, 18)]


def nan_outputs(c, where):
    """(got, want, mask): the cell's output with a NaN planted in X ('x': one coordinate of one point) or in A ('a': one element),
    the NaN-free expectation, and the outputs that have to be NaN"""
    d = MC.cell_data(c)
    want = expected_exact(c, d)
    m, n = d.A.shape
    k0, i0, j0 = d.X.shape[0] // 2, m // 2 + 1, n - 1
    y = np.zeros((m, d.X.shape[0]))
    if where == "x":
        d.X[k0, j0] = np.nan
        y[:, k0] = 1
    else:
        d.A[i0, j0] = np.nan
        y[i0, :] = 1
    mask = MC.layout(y, c.op) != 0 if c.op != "fbd" else (y[:, 0::2] + y[:, 1::2]).ravel() != 0
    (got,), count = run_cell(c, d, calls=1)
    return got[MC.GUARD:MC.GUARD + count], want, mask


@pytest.mark.xfail(strict=True, reason=NAN_REASON)
@pytest.mark.parametrize("where", ["x", "a"])
@pytest.mark.parametrize("c", NAN_CELLS, ids=lambda c: "%s-n%d-p%d" % (c.op, c.n, c.p))
def test_nan_is_contained_and_visible(c, where):
    got, want, mask = nan_outputs(c, where)
    assert MC.same_bits(got[~mask], want[~mask]), "another output moved"
    assert np.all(np.isnan(got[mask])), "nan-to-one: the outputs a NaN feeds are numbers"


@pytest.mark.parametrize("where", ["x", "a"])
@pytest.mark.parametrize("c", NAN_CELLS, ids=lambda c: "%s-n%d-p%d" % (c.op, c.n, c.p))
def test_nan_moves_no_other_output(c, where):
    """what holds today: the NaN stays in its point's / its row's outputs (which come out as numbers, +-1 - b or differences of them)"""
    got, want, mask = nan_outputs(c, where)
    assert MC.same_bits(got[~mask], want[~mask])
    assert np.all(np.isfinite(got[mask]))


def solve_both(O, A, b, x0):
    prob = W.TanhLinear(A, b)
    res, _ = prob.solve(x0)
    ctx = O.TanhLinearCtx(A.ctypes.data, b.ctypes.data)
    ro, _ = O.optimize(O.native_fn("wlc_tanh_linear_f"), A.shape[0], x0, fctx=C.addressof(ctx))
    return res, ro


def test_solve_from_a_nan_point_ends_as_the_oracles(oracle):
    """a NaN in x0 never reaches the model: both tiers refuse the point before the first residual"""
    rng = np.random.default_rng(3)
    A, b, x0 = rng.uniform(-1, 1, (500, 32)) * 0.3, rng.uniform(-1, 1, 500), rng.uniform(-1, 1, 32)
    x0[5] = np.nan
    res, ro = solve_both(oracle, A, b, x0)
    assert int(res.status) == ro.status and int(res.status) < 0 and res.iterations == 0


@pytest.mark.xfail(strict=True, reason=NAN_REASON)
def test_solve_with_a_nan_in_the_model_data_ends_as_the_oracles(oracle):
    """a NaN in A makes the host model's residual NaN from the first evaluation (tests/test_gpu_edge_cases.py::
    test_nan_residual_is_numeric_error: the same status as the oracle); the device model's residual is a number"""
    rng = np.random.default_rng(3)
    A, b, x0 = rng.uniform(-1, 1, (500, 32)) * 0.3, rng.uniform(-1, 1, 500), rng.uniform(-1, 1, 32)
    A[77, 3] = np.nan
    res, ro = solve_both(oracle, A, b, x0)
    assert ro.status < 0
    assert int(res.status) == ro.status


# ------------------------------------------------------------------------------------------------------------ Gaussian sum
def curve_call(name, dtype, t, data, X, count, kind=0, p=None):
    dt = np.dtype(dtype)
    stream = api.Stream()
    bufs = [api.DeviceBuffer(v) for v in (t, data, X)]
    ctx = W._CurveCtx(bufs[0].ptr, bufs[1].ptr, stream.handle, kind)
    fill = np.concatenate([MC.canary(MC.GUARD, dt, 1), MC.canary(count, dt, 0), MC.canary(MC.GUARD, dt, 2)])
    bY = api.DeviceBuffer(fill)
    args = [C.c_void_p(C.addressof(ctx)), C.c_size_t(len(t)), C.c_size_t(X.shape[-1])] + ([] if p is None else [C.c_size_t(p)])
    getattr(api.workloads_lib(), name)(*args, C.c_void_p(bufs[2].ptr), C.c_void_p(bY.ptr + MC.GUARD * dt.itemsize))
    stream.synchronize()
    out = bY.download()
    assert MC.same_bits(bufs[2].download(), X) and MC.same_bits(bufs[0].download(), t), "inputs changed"
    for b_ in bufs + [bY]:
        b_.free()
    stream.close()
    return out


def reference_rows(m):
    if m <= 257:
        return list(range(m))
    return sorted(set([0, 1, 2, m - 3, m - 2, m - 1]) | set(np.random.default_rng(m).integers(0, m, 250).tolist()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K", MC.GAUSS_K)
@pytest.mark.parametrize("m", MC.GAUSS_M)
def test_gauss_sum(m, K, dtype):
    n = 3 * K + 1
    rows = reference_rows(m)
    assert W.gauss_sum_class("f", m, n) == ("k_gauss_sum", K <= MC.KGAUSSMAX)
    per_point = {}
    for p in (7, 32):
        t, data, X = MC.gauss_inputs(m, K, p, dtype)
        ys = []
        for k in range(p):
            got = curve_call("wl_gauss_sum_f_" + ("d" if dtype == np.float64 else "s"), dtype, t, data, X[k], m)
            if k in (0, p - 1):                                  # an ordinary point and the one with the underflow and the far centre
                E = W.unary("exp", MC.gauss_arguments(t, X[k], K), dtype=dtype)
                want = MC.gauss_reference(t, data, X[k], K, E, rows)
                body = got[MC.GUARD:MC.GUARD + m]
                assert MC.same_bits(body[rows], want), ("values", p, k, np.flatnonzero(MC.bits(body[rows]) != MC.bits(want))[:5])
                if k == p - 1:
                    assert np.all(E[:, 0] == 0)                  # the tiny width: every exponential underflows
            MC.check_band(got, got[MC.GUARD:MC.GUARD + m], m)
            ys.append(got[MC.GUARD:MC.GUARD + m])
        per_point[p] = (t, data, X, np.stack(ys))
    if dtype != np.float64:
        return
    for p, (t, data, X, Y) in per_point.items():                # every layout of the batched kernel: the per-point kernel's bits
        assert W.gauss_sum_class("fb", m, n, p) == ("batched_pm", False)
        MC.check_band(curve_call("wl_gauss_sum_fb_d", dtype, t, data, X, m * p, p=p), Y.ravel(), m * p)
        fixed = K <= MC.KGAUSSMAX and (MC.gauss_blocks(m * p) * 256) % p == 0      # p = 32: always; p = 7: m = 255, 256 (7 workgroups)
        assert W.gauss_sum_class("fbr", m, n, p) == ("batched_rm", fixed)
        MC.check_band(curve_call("wl_gauss_sum_fbr_d", dtype, t, data, X, m * p, p=p), np.ascontiguousarray(Y.T).ravel(), m * p)


def test_gauss_sum_writes_nothing_for_nothing():
    t, data, X = MC.gauss_inputs(5, 5, 3)
    for name, m, p in (("wl_gauss_sum_f_d", 0, None), ("wl_gauss_sum_fb_d", 0, 3), ("wl_gauss_sum_fb_d", 5, 0), ("wl_gauss_sum_fbr_d", 0, 3),
                       ("wl_gauss_sum_fbr_d", 5, 0)):
        got = curve_call(name, np.float64, t[:m], data[:m], X[0] if p is None else X, 8, p=p)
        MC.check_band(got, MC.canary(8, np.dtype(np.float64), 0), 8)


# ------------------------------------------------------------------------------------------------------------ exponential decay
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 70000])
def test_exp_decay(m, kind, dtype):
    rng = np.random.default_rng([m, kind])
    t = rng.uniform(0, 3, m).astype(dtype)
    data = rng.standard_normal(m).astype(dtype)
    x = np.array([2.0, 1.5, 0.3][:2 + kind], dtype=dtype)
    got = curve_call("wl_exp_decay_f_" + ("d" if dtype == np.float64 else "s"), dtype, t, data, x, m, kind=kind)
    MC.check_band(got, got[MC.GUARD:MC.GUARD + m], m)
    E = W.unary("exp", MC.exp_decay_argument(t, x, kind), dtype=dtype)
    ref, bound = MC.exp_decay_reference(t, data, x, kind, E)
    ratio = float(np.max(np.abs(got[MC.GUARD:MC.GUARD + m].astype(MC.LD) - ref) / bound))
    print("exp_decay kind %d %s m = %d: largest error / bound %.3f" % (kind, np.dtype(dtype).name, m, ratio))
    assert ratio <= 1.0
