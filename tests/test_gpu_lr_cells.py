"""The read-only Broyden sweep's kernels (csrc/broyden_lr.h) at kernel level on the device: every cell of tests/lr_cases.py through
mir_lsq_lr_pass_* / mir_lsq_lr_flush_* on guarded buffers, once on exact-integer data (bits) and once on random data (derived
bounds, staged on the device's own intermediates; bit identities; a second call). lr_cases' docstring names the checks and holds
the derivations; tests/test_lr_cell_coverage.py shows on the CPU that the cells reach every instance and that each check catches
the mistake it is meant for."""
import numpy as np
import pytest

from mir_optim_amd import api
import lr_cases as K

pytestmark = pytest.mark.gpu

PASS = [c for c in K.CELLS if c.kind == "pass"]
FLUSH = [c for c in K.CELLS if c.kind == "flush"]
CHAIN = [c for c in K.CELLS if c.kind == "chain"]


def _pass_checks(cell, res, inp, exact):
    if cell.mode in K.NOGO:
        K.check_nogo(res, inp)
        return {}
    finished = cell.mode == "plain"
    if exact:
        K.check_exact_pass(res, inp, finished)
        K.check_bits(res, inp, finished)
        return {}
    ratios = {"u": K.check_u(res, inp), "reduced": K.check_reduced(res, inp)}
    if finished:
        ratios["JJ"], ratios["Jy"] = K.check_finish(res, inp)
    K.check_bits(res, inp, finished)
    K.check_sums(res, inp)
    return ratios


@pytest.mark.parametrize("cell", PASS, ids=K.cell_id)
def test_pass_cell(cell):
    if cell.m == K.M_GRID:
        assert api.lr_blocks(cell.m) == api.LR_MAX_BLOCKS, "this device has fewer than 256 compute units: the grid's upper limit is not reached"
    ex = K.exact_inputs(cell.m, cell.n, cell.k, cell.dtype, cell.count)
    _pass_checks(cell, K.run_pass(cell, ex), ex, True)
    inp = K.random_inputs(cell.m, cell.n, cell.k, cell.dtype, cell.count)
    res = K.run_pass(cell, inp)
    ratios = _pass_checks(cell, res, inp, False)
    print(K.cell_id(cell), "workgroups", res["nblk"], "error / bound", {a: round(v, 4) for a, v in ratios.items()})
    K.check_same(res, K.run_pass(cell, inp))


@pytest.mark.parametrize("cell", FLUSH, ids=K.cell_id)
def test_flush_cell(cell):
    ex = K.exact_inputs(cell.m, cell.n, cell.k, cell.dtype)
    K.check_exact_flush(K.run_flush(cell, ex), ex)
    inp = K.random_inputs(cell.m, cell.n, cell.k, cell.dtype)
    Jf = K.run_flush(cell, inp)
    print(K.cell_id(cell), "error / bound", round(K.check_flush(Jf, inp), 4))
    K.named("bits", np.array_equal(K.bits(Jf), K.bits(K.run_flush(cell, inp))), "a second call gave another J")


@pytest.mark.parametrize("cell", CHAIN, ids=K.cell_id)
def test_chain_cell(cell):
    ratios = K.chain(cell, K.run_pass, K.run_flush)
    print(K.cell_id(cell), "error / bound of JJ, Jy, the flushed J", [round(r, 4) for r in ratios])
