"""CPU tier of the scaled sweep's kernel-level tests (tests/lr_scaled_cases.py, run on the device by tests/test_gpu_lr_scaled.py):
the cell list reaches every scaled instance launch_broyden.hip compiles -- f64, NCP 1, 2, 4, 8, both load flavours, sweep and
flush -- through the library's own class function (mir_lsq_lr_class, host code), names what its axes say, and the numpy statement
of the scaling does what the header says, special values included."""
import numpy as np

import lr_scaled_cases as S


def test_cells_reach_exactly_the_scaled_instances():
    image = {}
    for c in S.CELLS:
        image.setdefault(S.cell_class(c), []).append(c)
    assert len(S.LISTED) == 16
    assert set(image) - S.LISTED == set(), "cells on instances the list does not have"
    assert S.LISTED - set(image) == set(), "listed instances no cell reaches"
    for (kern, ncp, vec), cells in image.items():           # the element-wise instances through a shifted even n, and an odd n
        if not vec:                                         # where the list of n has one (none between 129 and 255)
            assert {(c.n % 2, c.off) for c in cells} >= ({(1, 0), (0, 1)} if ncp <= 4 else {(0, 1)}), (kern, ncp)


def test_cell_list_is_what_its_axes_say():
    passes = [c for c in S.CELLS if c.kind == "pass"]
    flushes = [c for c in S.CELLS if c.kind == "flush"]
    assert S.NS == (1, 7, 32, 33, 64, 100, 127, 128, 130, 192, 256) and S.MS == (1, 3, 5, 129, 1031)
    for cells, ks in ((passes, {0, 1, 5, 15}), (flushes, {1, 2, 16})):
        assert {(c.n, c.m) for c in cells} == {(n, m) for n in S.NS for m in S.MS}
        assert {c.n for c in cells if c.off == 1} == {n for n in S.NS if n % 2 == 0}
        for n in S.NS:
            for m in S.MS:
                assert {c.k for c in cells if (c.n, c.m) == (n, m) and c.mode in ("plain", "")} >= ks
    for n in S.NS:
        for m in S.MS:
            modes = {c.mode for c in passes if (c.n, c.m) == (n, m)}
            assert modes == {"plain", S.GO, S.NOGO}                          # one go record and one no-go record
            assert any(c.poisoned for c in passes if (c.n, c.m) == (n, m)) == S.has_live_column(n)


def test_the_panels_carry_the_zeros_and_the_special_values():
    for n in S.NS:
        for m in S.MS:
            zc = S.collapsed_columns(n)
            assert 0 in zc and n - 1 in zc and n // 2 in zc
            for poisoned in ((False, True) if S.has_live_column(n) else (False,)):
                D, twh = S.panel_case(m, n, poisoned)
                assert D.shape == (m, n) and np.all(twh[zc] == 0) and np.count_nonzero(twh == 0) == len(zc)
                assert not np.all(np.isfinite(D[:, zc]))                      # a special value in a collapsed column
                live = [j for j in range(n) if j not in zc]
                assert np.all(np.isfinite(D[:, live])) != poisoned or not live
                J = S.scale_by_hand(D, twh)
                assert np.all(J[:, zc] == 0) and not np.any(np.signbit(J[:, zc]))     # reads as +0, NaN and Inf included
                if poisoned:
                    assert np.isnan(J[0, live[0]]) and np.isinf(J[m - 1, live[-1]])
                fin = np.isfinite(D)
                fin[:, zc] = False
                want = D * (1.0 / np.where(twh == 0, 1.0, twh))[None, :]
                assert np.array_equal(J[fin], want[fin])
