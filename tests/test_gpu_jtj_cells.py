"""Every instantiated J^T J kernel class at kernel level (jtj_cases.CELLS; tests/test_jtj_cell_coverage.py proves the list covers
launch_jtj.hip), through the guarded runner: buffers between NaN guard bands that must come back bit-identical, exact-integer
data that must come back bit-exact, random data inside the derived forward bounds of jtj_cases.product_bound /
broyden_reference, determinism, NaN localisation, and J one element off the 16-byte grid. Plain numpy references only.

Each test prints the largest error / bound ratio it saw ("ratio ..." lines, pytest -s); a ratio above 1 fails by construction.
Recorded on an MI355X, not asserted: product_bound 8.0e-3 (f64) and 6.5e-3 (f32) at m = 1001 / 1002, 0.10 / 0.11 at m = 66 / 67 and
up to 0.999 at m = 1 (one rounding against gamma_1: the bound is attained); broyden_reference's bound 0.46 (f64), 0.44 (f32)."""
import numpy as np
import pytest

from mir_optim_amd import api
import jtj_cases as K

pytestmark = pytest.mark.gpu

DT = {4: np.float32, 8: np.float64}


def ratio(err, bound):
    """max |err| / bound; an error where the bound is zero (an exactly zero sum of zero terms) must itself be zero"""
    err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
    assert not np.any(np.isnan(err)) and np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def check_products(tag, JJ, Jy, J_used, y, dtype):
    """symmetry bit for bit, and both products inside product_bound of the J they were formed from"""
    assert K.same_bits(JJ, np.ascontiguousarray(JJ.T))
    JJr, Jyr = K.ref_products(J_used, y)
    bJJ, bJy = K.product_bound(J_used, y, dtype)
    r = max(ratio(JJ - JJr, bJJ), ratio(Jy - Jyr, bJy))
    print(f"ratio product {np.dtype(dtype).name} {tag} {r:.3e}")
    assert r <= 1.0, (tag, r)


def run_plain_or_rewrite(cell, off):
    """assertions 1 to 3 for one cell at one alignment; -> the outputs on exact and on random data"""
    es, op, m, n, _ = cell
    dtype, rewrite, tag = DT[es], op == "rewrite", K.cell_id(cell)
    # 1. exact integers: bit-equal to the reference
    c = K.exact_case(m, n, dtype, rewrite)
    JJ, Jy, Ja = K.run_jtj(c["J"], c["y"], c["y_old"], c["dx"], dtype=dtype, j_offset_elems=off)
    assert K.same_bits(Ja, c["J_after"]), np.argwhere(Ja != c["J_after"])[:4]
    assert K.same_bits(JJ, c["JJ"]), np.argwhere(JJ != c["JJ"])[:4]
    assert K.same_bits(Jy, c["Jy"]), np.argwhere(Jy != c["Jy"])[:4]
    assert K.same_bits(JJ, np.ascontiguousarray(JJ.T))
    exact = (JJ, Jy, Ja)
    # 2. random normal data: inside the derived bounds
    r = K.random_case(m, n, dtype, rewrite)
    JJ, Jy, Ja = K.run_jtj(r["J"], r["y"], r["y_old"], r["dx"], dtype=dtype, j_offset_elems=off)
    if rewrite:
        ref, bound = K.broyden_reference(r["J"], r["y"], r["y_old"], r["dx"])
        rb = ratio(Ja - ref, bound)
        print(f"ratio broyden {np.dtype(dtype).name} {tag} {rb:.3e}")
        assert rb <= 1.0, (tag, rb)
    else:
        assert K.same_bits(Ja, r["J"])
    check_products(tag, JJ, Jy, Ja, r["y"], dtype)          # behind a rewrite: the products of the RETURNED J
    # 3. determinism
    again = K.run_jtj(r["J"], r["y"], r["y_old"], r["dx"], dtype=dtype, j_offset_elems=off)
    assert all(K.same_bits(a, b) for a, b in zip((JJ, Jy, Ja), again))
    return exact, (JJ, Jy, Ja)


def run_fd(cell, off, jout_off=0):
    """fd, fd_diff: J, JJ, Jy. fd_diff_keep: the call with J = NULL -- JJ and Jy held to the same references and bounds, and to the
    BITS of the fd_diff call on the same data (same grid, slabs and MFMA order); the panel comes back unchanged."""
    es, op, m, n, _ = cell
    diff, keep, tag = op != "fd", op == "fd_diff_keep", K.cell_id(cell)
    c = K.fd_case(m, n, diff, True)
    J, JJ, Jy = K.run_fd_jtj(c["panel"], c["twh"], c["y"], diff, off, jout_off, keep)
    assert K.same_bits(J, c["panel"] if keep else c["J"]) and K.same_bits(JJ, c["JJ"]) and K.same_bits(Jy, c["Jy"])
    assert K.same_bits(JJ, np.ascontiguousarray(JJ.T))
    exact = (J, JJ, Jy)
    r = K.fd_case(m, n, diff, False)
    J, JJ, Jy = K.run_fd_jtj(r["panel"], r["twh"], r["y"], diff, off, jout_off, keep)
    assert K.same_bits(J, r["panel"] if keep else r["J"])   # the Jacobian of ref_fill, bit for bit (keep: the panel, untouched)
    check_products(tag, JJ, Jy, r["J"], r["y"], np.float64)
    again = K.run_fd_jtj(r["panel"], r["twh"], r["y"], diff, off, jout_off, keep)
    assert all(K.same_bits(a, b) for a, b in zip((J, JJ, Jy), again))
    if keep:
        for data, got in ((c, exact), (r, (J, JJ, Jy))):
            Jw, JJw, Jyw = K.run_fd_jtj(data["panel"], data["twh"], data["y"], True, off, jout_off)
            assert K.same_bits(Jw, data["J"]) and K.same_bits(got[1], JJw) and K.same_bits(got[2], Jyw), tag
    return exact, (J, JJ, Jy)


@pytest.mark.parametrize("es", [4, 8])
@pytest.mark.parametrize("where", ["front", "slack", "back", "read-only payload"])
def test_the_guard_check_sees_one_changed_word(es, where):
    """the runner's own check: one word changed anywhere outside the payload (or inside a read-only one) fails finish()"""
    dtype = DT[es]
    payload = np.arange(37, dtype=dtype)
    g = K.Guarded(dtype, 37, payload, offset_elems=1)
    word = {"front": 0, "slack": g.start - 1, "back": g.total - 1, "read-only payload": g.start + 5}[where]
    assert same_after_roundtrip(K.Guarded(dtype, 37, payload, offset_elems=1), payload)
    g.buf.upload_at(word * es, np.array([K.NAN_BITS[es] ^ 1 if where != "read-only payload" else 0], dtype=K.UINT[es]))
    with pytest.raises(AssertionError):
        g.finish("probe", written=False)


def same_after_roundtrip(g, payload):
    return K.same_bits(g.finish("probe", written=False), payload)


def run_cell(cell, off, jout_off=0):
    return run_fd(cell, off, jout_off) if cell[1] in ("fd", "fd_diff", "fd_diff_keep") else run_plain_or_rewrite(cell, off)


@pytest.mark.parametrize("cell", [c for c in K.CELLS if c[4] == 0], ids=K.cell_id)
def test_cell(cell):
    run_cell(cell, 0)


@pytest.mark.parametrize("cell", [c for c in K.CELLS if c[4] == 1], ids=K.cell_id)
def test_cell_with_j_off_the_16_byte_grid(cell):
    """5. the same assertions with J (the difference panel) shifted by one element; exact integers: the bits of the aligned run;
    random data: the bits of the aligned run where the plan launches the same kernel on the same grid for both alignments"""
    es, op, m, n, _ = cell
    cu = 256
    pa, pu = api.jtj_plan(es, m, n, cu, op, True), api.jtj_plan(es, m, n, cu, op, False)
    assert pu["family"] != "ring8"                          # 16-byte LDS-DMA from an 8-byte-aligned address: not established, not run
    exact_u, random_u = run_cell(cell, 1)
    exact_a, random_a = run_cell(cell, 0)
    assert all(K.same_bits(a, b) for a, b in zip(exact_u, exact_a))
    if pa == pu:
        assert all(K.same_bits(a, b) for a, b in zip(random_u, random_a))


@pytest.mark.parametrize("cell", K.JOUT_OFFSET_CELLS, ids=K.cell_id)
def test_fd_diff_with_only_jout_off_the_16_byte_grid(cell):
    exact_u, random_u = run_cell(cell, 0, jout_off=1)
    exact_a, random_a = run_cell(cell, 0)
    assert all(K.same_bits(a, b) for a, b in zip(exact_u + random_u, exact_a + random_a))     # the same kernel reads the same panel


@pytest.mark.parametrize("cell", [c for c in K.CELLS if c[2] in K.NAN_MS and c[1] in ("plain", "rewrite") and c[4] == 0], ids=K.cell_id)
def test_nan_localisation(cell):
    """4. one NaN at J[m - 1, c], c neither first nor last, in the last row of a partial 4-row group (m % 4 == 3; the ring takes even
    m: m % 4 == 2), NaN guards behind J. plain: exactly row c and column c of J^T J and (J^T y)[c] are NaN, every other entry keeps
    its exact value. rewrite: exactly row m - 1 of J_after is NaN (J_i.dx is), every other row keeps its exact value; the products
    are those of the returned J, whose every column now holds a NaN. A tail row or a padding column that is multiplied by zero
    where it should be selected spreads the NaN and fails here."""
    es, op, m, n, _ = cell
    dtype, rewrite = DT[es], op == "rewrite"
    c = K.exact_case(m, n, dtype, rewrite)
    col = n // 2
    assert 0 < col < n - 1
    J = c["J"].copy()
    J[m - 1, col] = np.nan
    JJ, Jy, Ja = K.run_jtj(J, c["y"], c["y_old"], c["dx"], dtype=dtype)
    nan_rows = np.zeros(m, dtype=bool)
    nan_cols = np.zeros(n, dtype=bool)
    if rewrite:
        nan_rows[m - 1] = True
        nan_cols[:] = True
        assert np.array_equal(np.isnan(Ja), np.repeat(nan_rows[:, None], n, axis=1))
        assert K.same_bits(Ja[:m - 1], c["J_after"][:m - 1])
    else:
        nan_cols[col] = True
        assert K.same_bits(Ja, J)
    expect = nan_cols[:, None] | nan_cols[None, :]
    assert np.array_equal(np.isnan(JJ), expect), np.argwhere(np.isnan(JJ) != expect)[:4]
    assert np.array_equal(np.isnan(Jy), nan_cols)
    assert K.same_bits(JJ[~expect], c["JJ"][~expect]) and K.same_bits(Jy[~nan_cols], c["Jy"][~nan_cols])
