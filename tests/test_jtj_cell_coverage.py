"""CPU tier: every J^T J kernel instance launch_jtj.hip compiles is reached by a shape of jtj_cases.CELLS, the list
tests/test_gpu_jtj_cells.py runs on the GPU. INSTANTIATED is written out independently of jtj_plan<T>(); CELLS goes through the
library's own plan (mir_lsq_jtj_plan, host code). A plan change that adds an instance fails here until a shape is added."""
import numpy as np
import pytest

from mir_optim_amd import api
import jtj_cases as K

CUS = (7, 256)


def roles(ncb, es):
    regs = ncb * (ncb + 1) // 2 * 4 * (es // 4)          # as jtj_roles_rt: at most 96 accumulator VGPRs a wave
    return 1 if regs <= 96 else (2 if regs <= 192 else 4)


@pytest.mark.parametrize("cu", CUS)
def test_cells_cover_exactly_the_instantiated_kernels(cu):
    image = {}
    for cell in K.CELLS:
        key, p = K.cell_key(cell, cu)
        assert p["family"] != "none", cell
        image.setdefault(key, []).append(cell)
    run = {k for k, status in K.INSTANTIATED.items() if status == "run"}
    assert set(image) - run == set(), "cells on instances the universe does not list (or must not run)"
    assert run - set(image) == set(), "instantiated kernels no cell reaches"
    # ring8 keeps its 16-byte LDS-DMA for an unaligned J: listed, never run; fd_diff_keep on fdp's strided producer needs 4 GB of
    # panel a workgroup: listed, not run (the kernel instance is fd_diff's, which runs)
    unverified = {k for k, status in K.INSTANTIATED.items() if status != "run"}
    ring8 = {(8, op, "ring8", k, False, "offset") for op in ("plain", "rewrite") for k in range(9, 17)}
    keep4 = {(8, "fd_diff_keep", "fdp", k, False, "any") for k in range(1, 9)}
    assert unverified == ring8 | keep4
    assert all(K.INSTANTIATED[k].startswith("unverified_offset: ") for k in ring8)
    assert all(K.INSTANTIATED[k].startswith("unverified_4gb: ") and (8, "fd_diff", "fdp", k[3], False, "any") in run for k in keep4)
    assert not any(api.jtj_plan(es, m, n, cu, op, off == 0)["family"] == "ring8" for es, op, m, n, off in K.CELLS if off)


@pytest.mark.parametrize("cu", CUS)
def test_wide_cells_have_an_off_diagonal_job_and_stream_cells_every_role_count(cu):
    wide, seen = {}, {4: set(), 8: set()}
    for cell in K.CELLS:
        key, p = K.cell_key(cell, cu)
        if key[2] == "wide":
            wide[key] = wide.get(key, False) or p["jobs"] >= 3      # two tiles a side: job (1, 0) has ti != tj
        if key[2] == "stream":
            seen[key[0]].add(roles(p["ncb"], key[0]))
    assert len(wide) == 6 and all(wide.values()), wide
    assert seen == {8: {1, 2, 4}, 4: {1, 2}}


def test_cell_list_is_what_the_gpu_file_needs():
    for es, op, m, n, off in K.CELLS + K.JOUT_OFFSET_CELLS:
        assert es in (4, 8) and op in api.JTJ_OPS and m >= 1 and n >= 1 and off in (0, 1)
        assert es == 8 or op in ("plain", "rewrite")
    # per (family, block count) one row count near 1000; per family and type the small ones; NaN localisation per family and type
    big, small, nan = set(), {}, set()
    for cell in K.CELLS:
        key, _ = K.cell_key(cell, 256)
        if cell[2] in (K.M_ODD, K.M_EVEN):
            big.add(key)
        small.setdefault((key[0], key[1], key[2]), set()).add(cell[2])
        if cell[2] in K.NAN_MS and cell[1] in ("plain", "rewrite"):
            nan.add((key[0], key[2]))
    assert big == {k for k, s in K.INSTANTIATED.items() if s == "run"}
    for fam, ms in small.items():
        assert ms >= ({2, 66} if fam[2] == "ring8" else set(K.SMALL_MS)), (fam, ms)
    assert nan == {(8, "stream"), (4, "stream"), (8, "fdp"), (4, "pc32"), (8, "ring8"), (8, "fdp8"), (8, "wide"), (4, "wide")}


def test_guard_layout():
    assert K.GUARD_BYTES % 256 == 0 and K.GUARD_BYTES >= 4096
    for es, bits in K.NAN_BITS.items():
        v = np.array([bits], dtype=K.UINT[es]).view({4: np.float32, 8: np.float64}[es])
        assert np.isnan(v[0])


def test_references_on_a_hand_checked_case():
    """broyden_reference and product_bound against a case small enough to do by hand, and the generators' exactness claims"""
    J = np.array([[1.0, 2.0], [3.0, -1.0]]); y = np.array([1.0, -2.0]); yo = np.array([0.0, 1.0]); dx = np.array([0.5, -0.5])
    ref, bound = K.broyden_reference(J, y, yo, dx)
    # d = 2; t = (yo - y) + J dx = (-1 - 0.5, 3 + 2) = (-1.5, 5); u = (3, -10); J + u dx^T
    assert np.array_equal(np.asarray(ref, dtype=np.float64), [[2.5, 0.5], [-2.0, 4.0]])
    assert np.all(bound > 0) and np.all(bound < 1e-13)
    JJ, Jy = K.ref_products(J, y)
    assert np.array_equal(np.asarray(JJ, dtype=np.float64), [[10.0, -1.0], [-1.0, 5.0]]) and np.array_equal(np.asarray(Jy, dtype=np.float64), [-5.0, 4.0])
    bJJ, bJy = K.product_bound(J, y, np.float32)
    assert np.all(bJJ >= 2 * 2.0 ** -24 * np.abs(J).T @ np.abs(J)) and np.all(bJJ < 2.01 * 2.0 ** -24 * np.abs(J).T @ np.abs(J) * 1.01)
    for n in (1, 2, 3, 4, 7, 33, 300):
        dx = K.exact_dx(n)
        s = float(dx @ dx)
        assert s in (1.0, 0.5) and np.count_nonzero(dx) == (4 if n >= 4 else (2 if n >= 2 else 1))
    for dtype in (np.float32, np.float64):
        for m, n in ((67, 7), (1001, 33), (1002, 128)):
            c = K.exact_case(m, n, dtype, True)
            assert c["J_after"].dtype == dtype and np.array_equal(4 * c["J_after"], np.rint(4 * c["J_after"]))
            assert np.any(c["J_after"] != c["J"])
