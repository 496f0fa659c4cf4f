"""The decision kernel of the general solver's round, k_decide_chain (csrc/misc_kernels.h), ONE launch at a time with the solver's
geometry (M.lmDecide -> mir_lsq_decide_d / _s) between guard bands, against the walk of tests/decide_cases.py (written from
least_squares.d:1080-1161): every state field, x, dx_acc, the sums and the pinned mirror BIT FOR BIT, the inputs unchanged, every
band intact, every field the path does not assign with the bits it went in with, and a second launch on the outputs of the first.
The cells, the notation and the named assertions are decide_cases.py's; tests/test_decide_cell_coverage.py keeps on the CPU that
they reach every branch of the walk and that each planted mistake fails the assertion meant for it.

Measured on an MI355X: 377 tests of this file in under 2 s (the first launch of the process 0.5 s, every other test at most
0.01 s); no cell failed in either type or under either settings, and the oracle replays hold 8 / 8 / 55 rejections and
21 / 18 / 26 good acceptances (t3a f64, t3a f32, t3b f64; profiles/r22/decide_fd_cells.txt)."""
import numpy as np
import pytest

from mir_optim_amd import api
import decide_cases as D

pytestmark = pytest.mark.gpu

DT = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
SN = list(D.SETTINGS)


def both(cell_dtype, S, ops, **modes):
    got = D.device(cell_dtype, S, ops, **modes)
    want, path = D.walk(cell_dtype, S, ops, **modes)
    D.compare(got, want, mirror=modes.get("mirror", True))
    D.untouched(got, ops, D.assigned_fields(path))
    return got, want, path


@pytest.mark.parametrize("cell", [pytest.param(c, id=D.cell_id(c)) for c in D.CELLS])
def test_cell(cell):
    S = D.settings_of(cell.dtype, D.SETTINGS[cell.settings])
    ops = D.build(cell.chain, cell.dtype, cell.lam, cell.mu)
    modes = dict(check_grad=cell.check_grad, lambda_from_state=cell.lambda_from_state, seq=77)
    got, want, path = both(cell.dtype, S, ops, **modes)
    st = got["state"]
    assert st["jy_inf"] == ops["state"]["jy_inf"] and st["pad0"] == ops["state"]["pad0"] and st["seq"] == ops["state"]["seq"]
    assert got["host_state"]["seq"][0] == 77
    if "g" == cell.chain[0] and cell.check_grad:               # the exit before anything else: nothing consumed, lambda not taken
        assert st["decision"][0] == api.LM_DECIDE_GRAD_SMALL and st["consumed"][0] == 0 and st["lambda"][0] == cell.dtype(cell.lam)
    if "g" in cell.chain and not (cell.chain[0] == "g" and cell.check_grad):
        assert st["decision"][0] == api.LM_DECIDE_ACCEPT and st["accepted_k"][0] == len(cell.chain) - 1
    if "X" in cell.chain:                                      # nothing behind the acceptance reaches the state but coop_rescued
        assert (st["accepted_k"][0], st["consumed"][0], st["qp_status"][0], st["coop_rescued"][0]) == (2, 3, 0, 2)
    if "Z" in cell.chain:
        k = cell.chain.index("Z")
        assert got["sums"][k] == cell.dtype(D.RESIDUAL)
    # a second launch on the outputs of the first behaves as the reference does on the same inputs
    again = dict(ops, state=got["state"], sums=got["sums"], x=got["x"], dx_acc=got["dx_acc"])
    both(cell.dtype, S, again, **modes)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("sname", SN)
@pytest.mark.parametrize("chain", ["A", "R", "RRAXxXxX", "ZRA", "F"])
def test_without_a_mirror_the_device_results_are_the_same(chain, sname, dtype):
    S = D.settings_of(dtype, D.SETTINGS[sname])
    ops = D.build(list(chain), dtype, D.LAM[sname], 1.0)
    a, _, _ = both(dtype, S, ops, mirror=True)
    b, _, _ = both(dtype, S, ops, mirror=False)
    for k in ("state", "sums", "x", "dx_acc"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("i,n", list(enumerate(D.NS)))
def test_the_accepted_rows_arrive_at_every_n(i, n, dtype):
    """n across the copy loop's stride of 256, a different accepted index a cell; and a ladder without an acceptance"""
    S = D.settings_of(dtype, {})
    chain = ["R"] * i + ["A"] + ["X"] * (7 - i)
    ops = D.build(chain, dtype, 0.125, 1.0, n=n)
    got, _, _ = both(dtype, S, ops)
    assert got["state"]["accepted_k"][0] == i
    for out, rows in (("x", "trial"), ("host_x", "trial"), ("dx_acc", "dx_chain")):
        assert got[out].tobytes() == ops[rows][i].tobytes(), out
    ops = D.build(["R"] * (i + 1), dtype, 0.125, 1.0, n=n)
    got, _, _ = both(dtype, S, ops)
    assert got["x"].tobytes() == ops["x"].tobytes() and got["dx_acc"].tobytes() == ops["dx_acc"].tobytes()
    assert set(got["host_x"].tobytes()) == {0xFF}


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("nparts", D.NPARTS)
def test_the_second_stage_of_the_sums(nparts, dtype):
    """exact-integer partials behind which the slots hold NaN: the sums are exact; random partials: the 32-range order to the bit"""
    S = D.settings_of(dtype, {})
    chain = ["R", "G", "Z", "I", "E", "A", "X", "x"]
    ops = D.build(chain, dtype, 0.125, 1.0, nparts=nparts, seed=nparts)
    got, _, _ = both(dtype, S, ops)
    plain = D.build(chain, dtype, 0.125, 1.0)
    for k, tok in enumerate(chain):
        if tok not in "GXx":                                   # (a guard's and the garbage's sums are whatever their partials hold)
            want = dtype(D.RESIDUAL) if tok == "Z" else plain["sums"][k]
            assert got["sums"][k] == want, (k, tok)
    assert got["state"]["accepted_k"][0] == 5
    rng = np.random.default_rng(nparts)
    ops = D.build(["R", "R", "R"], dtype, 0.125, 1.0, nparts=nparts)
    ops["partials"][:, :nparts] = (200.0 + rng.standard_normal((3, nparts)) * 50.0).astype(dtype)
    got, _, _ = both(dtype, S, ops)
    for k in range(3):
        assert D.same_bits(got["sums"][k:k + 1], np.array([D.reduce32(ops["partials"][k], nparts)], dtype=dtype))


SPEC_BASE = dict(maxLambda=64.0)
SPEC_STOPS = [   # (name, settings on top of the base, maxIterations, record fields, tokens it applies to)
    ("converged", dict(maxGoodResidual=90.0), 1000, {}, "AP"),
    ("last_iteration", {}, 26, {}, "AP"),
    ("lambda_above_max", dict(maxLambda=0.01), 1000, {}, "AP"),
    ("lambda_below_min", dict(minLambda=1000.0, maxLambda=1e6), 1000, {}, "P"),
    ("step_at_abs_tolerance", dict(absTolerance=2.0), 1000, dict(new_dx_dot=4.0), "AP"),
    ("step_at_rel_tolerance", dict(relTolerance=25.0), 1000, dict(new_dx_dot=4.0, trial_xnorm=50.0), "AP"),
    ("flag_x_nan", {}, 1000, dict(flags=D.FLAG_X_NAN), "AP"),
    ("flag_grad_small", {}, 1000, dict(flags=D.FLAG_GRAD), "AP"),
    ("flag_dx_nan", {}, 1000, dict(flags=D.FLAG_DX_NAN), "AP"),
    ("flag_guard", {}, 1000, dict(flags=D.FLAG_GUARD), "AP"),
    ("flag_null", {}, 1000, dict(flags=D.FLAG_NULL), "AP"),
    ("qp_failed", {}, 1000, dict(qp_status=1), "AP"),
]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("sname", SN)
@pytest.mark.parametrize("tok", ["A", "P"])
def test_spec_ok(tok, sname, dtype):
    def run(chain, over, max_it, fields, spec_static=True):
        S = D.settings_of(dtype, dict(D.SETTINGS[sname], **dict(SPEC_BASE, **over)))
        ops = D.build(chain, dtype, D.LAM[sname], 1.0)
        for k, v in fields.items():
            ops["rec"][0][k] = v
        got, _, path = both(dtype, S, ops, spec_static=spec_static, maxIterations=max_it)
        return int(got["state"]["spec_ok"][0]), path
    assert run([tok], {}, 1000, {}) == (1, [{"A": "rate_good", "P": "rate_poor"}[tok], "spec_go"])
    assert run([tok], {}, 27, {})[0] == 1                        # iterations + 1 < maxIterations
    assert run([tok], dict(absTolerance=1.99), 1000, dict(new_dx_dot=4.0))[0] == 1
    for name, over, max_it, fields, toks in SPEC_STOPS:
        if tok in toks:
            assert run([tok], over, max_it, fields)[0] == 0, name
    assert run([tok], {}, 1000, {}, spec_static=False)[0] == 0
    for chain in (["N"], ["R"], ["R", tok]):                    # no prediction, a rejection, an acceptance that is not entry 0
        assert run(chain, {}, 1000, {})[0] == 0, chain


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("sname", SN)
@pytest.mark.parametrize("mu", [1.0, D.MU_ODD])
def test_lambda_after_j_rejections_is_the_hosts_ladder(mu, sname, dtype):
    """the ladder the host loop builds for speculative solves (LM_REJECT on a copy of lambda and mu, once an entry), restated"""
    S = D.settings_of(dtype, D.SETTINGS[sname])
    inc = dtype(S.lambdaIncrease)
    l2, m2 = dtype(D.LAM[sname]), dtype(mu)
    for j in range(1, 9):
        with np.errstate(over="ignore"):
            l2 = l2 * (inc * m2)
            m2 = m2 * dtype(2)
        chain = [("G" if (k % 3 == 1) else "R") for k in range(j)]
        got, _, _ = both(dtype, S, D.build(chain, dtype, D.LAM[sname], mu))
        assert D.same_bits(got["state"]["lambda"], np.array([l2], dtype=dtype)) and got["state"]["mu"][0] == m2, j


@pytest.mark.parametrize("name,dtype", D.REPLAY, ids=["%s-%s" % (n, np.dtype(d).name) for n, d in D.REPLAY])
def test_oracle_replay(oracle, name, dtype):
    rejections, good = D.replay(D.device, name, dtype)
    print("replayed %d rejections and %d good acceptances of the oracle's trace through the kernel" % (rejections, good))
