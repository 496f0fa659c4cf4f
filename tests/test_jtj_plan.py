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


def expected_family(es, m, n, op, aligned):
    f64 = es == 8
    if op in ("fd", "fd_diff"):                      # the fused finite-difference kernels: f64, n <= 256
        if not f64 or n > 256:
            return "none"
        if n <= 128:
            return "fdp"
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
        if op in ("fd", "fd_diff"):
            uncovered = es == 4 or n > 256 or (op == "fd_diff" and 128 < n <= 256 and n % 64 != 0)
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
        cap = {"stream": 4 * cu, "fdp": (2 if tuned else 4) * cu, "pc32": 2 * cu, "ring8": cu, "fdp8": cu,
               "wide": max(1, 4 * cu // p["jobs"])}[fam]
        assert 1 <= p["grid"] <= cap, row
        assert p["lds"] <= 160 * 1024, row
        assert p["slabs"] == p["grid"] * p["jobs"] and p["workspace_slab_elems"] >= p["slabs"] * p["slab_len"], row
        # the block count is one the kernel is instantiated for, and it covers n
        if fam == "wide":
            tiles = (blocks + 3) // 4
            assert ncb == blocks and p["jobs"] == tiles * (tiles + 1) // 2 and p["slab_len"] == 68 * 64 and p["reduce_ncb"] == 0, row
            continue
        if fam == "fdp8":
            assert ncb == 2 * ((n + 31) // 32) and ncb in ((12, 16) if op == "fd_diff" else (10, 12, 14, 16)), row
        else:
            assert ncb == blocks and ncb in (range(9, 17) if fam == "ring8" else range(1, 9)), row
        assert p["jobs"] == 1 and p["reduce_ncb"] == ncb and p["slab_len"] == (ncb * (ncb + 1) // 2 * 4 + ncb) * 64, row
        flat = fam == "fdp" and op != "fd" and (n % 2 == 1 or not aligned or (op == "fd_diff" and n % 16 != 0))
        assert p["flat"] == flat, row


def test_unaligned_fallback_fits_the_workspace_of_the_aligned_plan():
    """the slab buffer is sized before the pointer is known: same workspace figure for both alignments"""
    for es, n, m, cu, op, _ in ROWS[::2]:
        assert api.jtj_plan(es, m, n, cu, op, True)["workspace_slab_elems"] == api.jtj_plan(es, m, n, cu, op, False)["workspace_slab_elems"]


def test_bad_arguments():
    for args in ((2, 10, 4, 256, "plain"), (8, 0, 4, 256, "plain"), (8, 10, 0, 256, "plain"), (8, 10, 4, 0, "plain")):
        with pytest.raises(ValueError):
            api.jtj_plan(*args)
