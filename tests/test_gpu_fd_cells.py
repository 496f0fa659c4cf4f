"""The finite-difference and bookkeeping kernels of csrc/misc_kernels.h one launch at a time between guard bands -- k_fd_points
(M.fdPoints), k_fd_fill / k_fd_fill_col (M.fdFill), k_sumsq_partial + k_sumsq_final + k_init_state + k_reset_mu (M.entryState) and
k_unpack_grad (M.unpackGrad) -- against the numpy references of tests/fd_cases.py: bit for bit everywhere but the random sums of
squares, which are held to the bound derived there (tests/test_decide_cell_coverage.py checks the references on the CPU).

Measured on an MI355X: 100 tests of this file in well under a second; random sums of squares at most 0.047 (float32) and 0.055
(float64) of their bound over m = 1 .. 131077 (profiles/r22/decide_fd_cells.txt)."""
import numpy as np
import pytest

from mir_optim_amd import api
import decide_cases as D
import fd_cases as F

pytestmark = pytest.mark.gpu

DT = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
same = D.same_bits


# ---------------------------------------------------------------------------------------------------------------- fd_points
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", F.POINT_NS)
def test_fd_points(n, dtype):
    for bounds, shift, eps in (("inf", 0, F.EPS), ("finite", 0, F.EPS), ("finite", 4, F.EPS), ("finite", 1, F.EPS_LARGE), ("finite", 3, F.EPS_LARGE)):
        x, lo, up = F.points_inputs(n, dtype, bounds, shift)
        for with_base in (False, True):
            got = api.fdPoints(x, lo, up, eps, dtype=dtype, with_base=with_base)
            X, twh = F.points_reference(x, lo, up, eps, with_base)
            what = (bounds, shift, eps, with_base)
            assert got["guard"] == -1, what
            assert same(got["X"], X), what
            assert same(got["twh"], twh), what
            assert same(got["twh_host"], got["twh"]), what         # the host's copy of the width arithmetic agrees with the device's
            if bounds == "finite":
                kind = (np.arange(n) + shift) % 6
                assert np.all(got["twh"][kind == 4] == 0) and np.all(got["twh"][kind != 4] > 0), what
                if eps == F.EPS_LARGE:                              # both sides clamp: the width is the box's
                    assert same(got["twh"], up - lo), what


# ---------------------------------------------------------------------------------------------------------------- fd_fill
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", F.FILL_NS)
@pytest.mark.parametrize("m", F.FILL_MS)
def test_fd_fill(m, n, dtype):
    for j0, pc in F.panels(n):
        for ldy in (m, m + 3):
            Y, twh, J = F.fill_inputs(m, n, j0, pc, ldy, dtype)
            got = api.fdFill(Y, twh, J, j0, pc, dtype=dtype)
            want = F.fill_reference(Y, twh, J, j0, pc)
            what = (j0, pc, ldy)
            assert got["guard"] == -1, what
            assert same(got["J"], want), (what, np.argwhere(D.bits(got["J"]) != D.bits(want))[:4])
            for j in F.collapsed_columns(m, j0, pc):                # an exact +0, the NaN rows of the panel not read
                assert not got["J"][:, j].any() and not np.signbit(got["J"][:, j]).any(), what
            outside = np.ones(n, bool)
            outside[j0:j0 + pc] = False
            assert np.all(got["J"][:, outside] == dtype(F.FILL_SENTINEL)), what


@pytest.mark.parametrize("dtype", DT)
def test_fd_fill_propagates_infinities_and_nans(dtype):
    m, n = 65, 33
    Y, twh, J = F.fill_inputs(m, n, 0, n, m + 3, dtype, special=True)
    got = api.fdFill(Y, twh, J, 0, n, dtype=dtype)
    want = F.fill_reference(Y, twh, J, 0, n)
    assert got["guard"] == -1 and same(got["J"], want)
    assert np.isinf(want).sum() >= 2 and np.isnan(want).sum() >= 2


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("m", F.FILL_MS)
def test_fd_fill_col(m, dtype):
    for n in (1, 33):
        for j in sorted({0, n - 1}):
            for zero in (False, True):
                Y, twh, J = F.fill_inputs(m, n, j, 1, m, dtype, seed=j)
                twh[j] = 0 if zero else dtype(2.0 ** -19 * 1.375)
                if zero:
                    Y[:] = np.nan
                elif np.isnan(Y).any():
                    Y[:] = np.random.default_rng(m).standard_normal(Y.shape).astype(dtype)
                got = api.fdFill(Y, twh, J, j, 1, dtype=dtype, col=True)
                assert got["guard"] == -1 and same(got["J"], F.fill_reference(Y, twh, J, j, 1)), (n, j, zero)
                if zero:
                    assert not got["J"][:, j].any() and not np.signbit(got["J"][:, j]).any()


# ---------------------------------------------------------------------------------------------------------------- entry state
def check_entry_state(got, dtype, seq, total):
    st = got["state"]
    assert st["lambda"][0] == 0 and st["mu"][0] == 1 and same(st["residual"], np.array([total], dtype=dtype))
    for k in st.dtype.names:
        if k not in ("lambda", "mu", "residual"):
            assert not st[k].view(np.uint32 if st[k].itemsize == 4 else np.uint64).any(), k
    for k in st.dtype.names:
        if k != "seq":
            assert same(got["host_state"][k], st[k]), k
    assert got["host_state"]["seq"][0] == seq and got["guard"] == -1


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("m", F.STATE_MS)
def test_entry_state(m, dtype):
    assert api.sumsq_blocks(m) == F.blocks_by_hand(m)
    st2 = F.distinct_state(dtype)
    v = F.exact_vectors(m, dtype)
    got = api.entryState(v, st2, dtype=dtype, seq=5 + m)
    exact = [int((v[k].astype(np.int64) ** 2).sum()) for k in range(2)]
    assert got["sum"] == exact[0] and float(got["partials"].astype(np.float64).sum()) == exact[0]
    check_entry_state(got, dtype, 5 + m, got["sum"])
    assert same(got["partials2"][0], got["partials"]) and got["sums2"].tolist() == exact          # gridDim.y = 2: vstride, pstride
    for k in st2.dtype.names:                                                                      # the forced refresh: mu alone
        assert same(got["st2"][k], np.array([1], dtype=dtype) if k == "mu" else st2[k]), k
    v = F.random_vectors(m, dtype)
    got = api.entryState(v, st2, dtype=dtype, seq=9)
    check_entry_state(got, dtype, 9, got["sum"])
    assert same(got["sums2"][:1], np.array([got["sum"]], dtype=dtype)) and same(got["partials2"][0], got["partials"])
    for k in range(2):
        ref = F.fsum_squares(v[k])
        err = abs(float(got["sums2"][k]) - ref) / ref
        print("m = %d %s vector %d: error / bound %.3f (chain of %d roundings)" % (m, np.dtype(dtype).name, k, err / F.bound(m, dtype), F.chain_length(m)))
        assert err <= F.bound(m, dtype), (k, err, F.bound(m, dtype))


# ---------------------------------------------------------------------------------------------------------------- unpack_grad
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", F.UNPACK_NS)
def test_unpack_grad(n, dtype):
    st = F.distinct_state(dtype)
    for where in F.UNPACK_MAX:
        packed = F.unpack_inputs(n, dtype, where)
        got = api.unpackGrad(packed, n, st, dtype=dtype)
        JJ, Jy, jy_inf = F.unpack_reference(packed, n)
        assert got["guard"] == -1, where
        assert same(got["JJ"], JJ) and same(got["Jy"], Jy), where
        assert got["state"]["jy_inf"][0] == jy_inf and jy_inf == (0 if where == "zero" else 1e6), where
        for k in st.dtype.names:
            if k != "jy_inf":
                assert same(got["state"][k], st[k]), (where, k)
