"""CPU tier: which J^T J kernel runs for a shape and an operation -- the table of csrc/jtj_plan.h as data, through the host-only
entry mir_lsq_jtj_plan (no GPU needed: num_cu is an argument). The expectation below is written independently of jtj_plan<T>();
a kernel choice that changes on purpose changes `expected_family` (and the header's table) with it."""
import itertools

import pytest

from mir_optim_amd import api

NS = (1, 2, 3, 15, 16, 17, 31, 64, 100, 126, 127, 128, 129, 144, 160, 192, 200, 208, 250, 255, 256, 257, 512, 1024)
MS = (1, 2, 63, 64, 4097, 100000, 1000000, 1000001)
CUS = (7, 256)
ROWS = list(itertools.product((8, 4), NS, MS, CUS, api.JTJ_OPS, (True, False)))


def rows_span_4gb(m, n, grid):
    """the rows of one workgroup of the fused FD kernel at n <= 128 -- ceil(ceil(m / 32) / grid) stages of 32 rows -- as bytes of the
    difference panel: do they reach 4 GB? (k_jtj_fdp_nw addresses them with 32-bit offsets)"""
    stages = -(-m // 32)
    return -(-stages // grid) * 32 * n * 8 >= 2 ** 32


def expected_family(es, m, n, op, aligned):
    f64 = es == 8
    if op in ("fd", "fd_diff", "fd_diff_keep"):      # the fused finite-difference kernels: f64, n <= 256
        if not f64 or n > 256:
            return "none"
        if n <= 128:
            # the store-free kernel: the panel kept as J, whole 128-byte rows on the 16-byte grid (no row of ROWS spans 4 GB)
            return "fdp_nw" if op == "fd_diff_keep" and n % 16 == 0 and aligned else "fdp"
        return "fdp8" if op == "fd" or n % 64 == 0 else "none"
    if n > 256 or (not f64 and n > 128):
        return "wide"
    if n > 128:                                      # f64: the ring's grid, else fdp8's plain flavour / tile pairs behind the rewrite
        if n % 16 == 0 and m % 2 == 0:
            return "ring8"
        return "fdp8" if op == "plain" else "wide"
    if op == "rewrite":
        return "stream"
    if f64:
        return "fdp"
    return "pc32" if n % 4 == 0 and aligned else "stream"


def test_family_per_shape_and_operation():
    for es, n, m, cu, op, aligned in ROWS:
        assert api.jtj_plan(es, m, n, cu, op, aligned)["family"] == expected_family(es, m, n, op, aligned), (es, m, n, cu, op, aligned)


def test_fused_fd_coverage():
    for es, n, m, cu, op, aligned in ROWS:
        if op in ("fd", "fd_diff", "fd_diff_keep"):
            uncovered = es == 4 or n > 256 or (op != "fd" and 128 < n <= 256 and n % 64 != 0)
            assert (api.jtj_plan(es, m, n, cu, op, aligned)["family"] == "none") == uncovered, (es, m, n, op)


def test_launch_invariants():
    for es, n, m, cu, op, aligned in ROWS:
        p = api.jtj_plan(es, m, n, cu, op, aligned)
        fam, ncb, row = p["family"], p["ncb"], (es, m, n, cu, op, aligned, p)
        if fam == "none":
            continue
        blocks = (n + 15) // 16
        # grid: at least one workgroup, at most the family's share of the chip
        tuned = n % 16 == 0 and m % 2 == 0            # fdp: two workgroups per CU on these, else k_jtj's grid
        cap = {"stream": 4 * cu, "fdp": (2 if tuned else 4) * cu, "fdp_nw": (2 if tuned else 4) * cu, "pc32": 2 * cu, "ring8": cu,
               "fdp8": cu, "wide": max(1, 4 * cu // p["jobs"])}[fam]
        assert fam != "fdp_nw" or not rows_span_4gb(m, n, p["grid"]), row
        assert 1 <= p["grid"] <= cap, row
        assert p["lds"] <= 160 * 1024, row
        assert p["slabs"] == p["grid"] * p["jobs"] and p["workspace_slab_elems"] >= p["slabs"] * p["slab_len"], row
        # the block count is one the kernel is instantiated for, and it covers n
        if fam == "wide":
            tiles = (blocks + 3) // 4
            assert ncb == blocks and p["jobs"] == tiles * (tiles + 1) // 2 and p["slab_len"] == 68 * 64 and p["reduce_ncb"] == 0, row
            continue
        if fam == "fdp8":
            assert ncb == 2 * ((n + 31) // 32) and ncb in ((12, 16) if op in ("fd_diff", "fd_diff_keep") else (10, 12, 14, 16)), row
        else:
            assert ncb == blocks and ncb in (range(9, 17) if fam == "ring8" else range(1, 9)), row
        assert p["jobs"] == 1 and p["reduce_ncb"] == ncb and p["slab_len"] == (ncb * (ncb + 1) // 2 * 4 + ncb) * 64, row
        flat = fam == "fdp" and op != "fd" and (n % 2 == 1 or not aligned or (op in ("fd_diff", "fd_diff_keep") and n % 16 != 0))
        assert p["flat"] == flat, row
        if op == "fd_diff_keep":                      # fd_diff's launch, whichever of the two kernels runs it
            q = api.jtj_plan(es, m, n, cu, "fd_diff", aligned)
            assert {k: v for k, v in p.items() if k != "family"} == {k: v for k, v in q.items() if k != "family"}, row
            assert fam == q["family"] or (fam == "fdp_nw" and q["family"] == "fdp" and not p["flat"]), row


@pytest.mark.parametrize("n", [128, 16])
@pytest.mark.parametrize("cu", [1, 7])
def test_store_free_kernel_ends_where_a_workgroups_rows_span_4gb(n, cu):
    """fd_diff_keep is fdp_nw as long as ceil(ceil(m / 32) / grid) * 32 * n * 8 < 2^32 and fd_diff's entry (fdp, strided producer)
    from the first m past that; the grid is the plan's own. m is only a number here: nothing is allocated."""
    def keep(m):
        return api.jtj_plan(8, m, n, cu, "fd_diff_keep", True)
    # At these sizes the grid has long reached its cap, which depends on the parity of m alone (fdp's tuned grid takes even m). Per
    # parity the largest m with ceil(ceil(m / 32) / grid) <= per_max, the most 32-row stages below 4 GB; the larger of the two is the last
    # m of fdp_nw: its successors of either parity are past their own parity's last.
    per_max = (2 ** 32 - 1) // (32 * n * 8)
    grids = [keep(2 ** 40 + parity)["grid"] for parity in (0, 1)]
    m_last = max(per_max * grids[parity] * 32 - (parity != 0) for parity in (0, 1))
    per_wg = ("lds", "slab_len", "ncb", "jobs", "reduce_ncb", "flat")                  # what does not depend on the grid
    figures = per_wg + ("grid", "slabs", "workspace_slab_elems")
    below = keep(m_last)
    assert below["grid"] == grids[m_last % 2] and not rows_span_4gb(m_last, n, below["grid"])
    assert below["family"] == "fdp_nw" and not below["flat"]
    for m in (m_last + 1, m_last + 2):                # the first m past it, and the first of m_last's own parity: the same grid
        above = keep(m)
        assert above["grid"] == grids[m % 2] and rows_span_4gb(m, n, above["grid"]), (m, above)
        assert above["family"] == "fdp" and not above["flat"], (m, above)
        assert [above[k] for k in per_wg] == [below[k] for k in per_wg], (m, above, below)
        assert above == api.jtj_plan(8, m, n, cu, "fd_diff", True)
    assert [keep(m_last + 2)[k] for k in figures] == [below[k] for k in figures]
    # an unaligned panel takes the flat producer on both sides of the boundary
    for m in (m_last, m_last + 1):
        u = api.jtj_plan(8, m, n, cu, "fd_diff_keep", False)
        assert u["family"] == "fdp" and u["flat"] == 1 and u == api.jtj_plan(8, m, n, cu, "fd_diff", False)


def test_unaligned_fallback_fits_the_workspace_of_the_aligned_plan():
    """the slab buffer is sized before the pointer is known: same workspace figure for both alignments"""
    for es, n, m, cu, op, _ in ROWS[::2]:
        assert api.jtj_plan(es, m, n, cu, op, True)["workspace_slab_elems"] == api.jtj_plan(es, m, n, cu, op, False)["workspace_slab_elems"]


def test_bad_arguments():
    for args in ((2, 10, 4, 256, "plain"), (8, 0, 4, 256, "plain"), (8, 10, 0, 256, "plain"), (8, 10, 4, 0, "plain")):
        with pytest.raises(ValueError):
            api.jtj_plan(*args)
