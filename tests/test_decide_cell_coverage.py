"""CPU tier of the decision and bookkeeping cells (tests/decide_cases.py and tests/fd_cases.py, run on the device by
tests/test_gpu_decide_cells.py and tests/test_gpu_fd_cells.py): the chains reach every decision value, every break and continue
of the walk and all three ratings under both settings -- asserted on the reference's own path record; the restated reject and
rate rules agree bit for bit with the shim library of tests/test_lm_rules.py; the oracle's trace replays through the reference;
each planted mistake in the reference fails the assertion named for it; the vectorised FD references agree with per-element
loops; and a numpy restatement of the two-stage sum of squares stays inside the derived bound in three orders."""
import ctypes as C

import numpy as np
import pytest

from mir_optim_amd import api
import decide_cases as D
import fd_cases as F
from test_lm_rules import shim  # noqa: F401  (the fixture that builds and loads liblm_rules_shim.so)

DT = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


def run(cell, plant=None):
    S = D.settings_of(cell.dtype, D.SETTINGS[cell.settings])
    ops = D.build(cell.chain, cell.dtype, cell.lam, cell.mu)
    res, path = D.walk(cell.dtype, S, ops, check_grad=cell.check_grad, lambda_from_state=cell.lambda_from_state, plant=plant)
    return ops, res, path


def test_the_state_layout():
    assert api.lm_state_dtype(np.float64).itemsize == 160 and api.lm_state_dtype(np.float32).itemsize == 108
    for dt in (np.float32, np.float64):
        t = api.lm_state_dtype(dt)
        assert t.names[:12] == api.LM_STATE_FLOATS and t.fields["qp_status"][1] == 12 * np.dtype(dt).itemsize
        assert t.fields["spec_ok"][1] == 12 * np.dtype(dt).itemsize + 56


def test_chains_reach_every_branch_of_the_walk():
    seen = {}
    for c in D.CELLS:
        ops, res, path = run(c)
        D.compare(res, res)
        D.untouched(res, ops, D.assigned_fields(path))
        for dt_sn in [(c.dtype, c.settings)]:
            seen.setdefault(dt_sn, {"paths": set(), "decisions": set()})
            seen[dt_sn]["paths"] |= set(path)
            seen[dt_sn]["decisions"].add(int(res["state"]["decision"][0]))
    assert len(seen) == 4
    for key, s in seen.items():
        assert s["decisions"] == {1, 2, 3, 4, 5}, key
        # the four breaks before an acceptance, the two continues, the break without a prediction, the three ratings (each ends in
        # the last break), the null step and the ladder that runs out
        assert s["paths"] == {"grad_exit", "qp_failed", "dx_nan", "not_finite", "guard", "reject", "no_prediction", "rate_poor", "rate_mid",
                              "rate_good", "null", "ladder_exhausted"}, key
    assert len(set(D.CELLS)) == len(D.CELLS)
    singles = {c.chain[0] for c in D.CELLS if len(c.chain) == 1}
    assert singles == set(D.SINGLES)
    named = ["RRRRRRRR", "GRGRGRGA", "RRRM", "ZZZ", "ZRA", "RZ", "ZR", "RRQ1", "GD", "RF", "EP", "RRAXxXxX"]
    assert set(named) <= {"".join(c.chain) for c in D.CELLS}


@pytest.mark.parametrize("dtype", DT)
def test_what_each_token_does(dtype):
    """the notation against the walk: decision, accepted index and counters of every single token"""
    want = {"A": (2, 0, 1, 0, 0), "M": (2, 0, 1, 0, 0), "P": (2, 0, 1, 0, 0), "N": (3, 0, 1, 0, 0), "N-": (3, 0, 1, 0, 0), "Nn": (3, 0, 1, 0, 0),
            "R": (1, -1, 1, 1, 0), "E": (1, -1, 1, 1, 0), "I": (1, -1, 1, 1, 0), "F": (4, -1, 1, 0, 0), "G": (1, -1, 0, 0, 1),
            "Z": (1, -1, 1, 1, 0), "Q1": (4, -1, 0, 0, 0), "Q2": (4, -1, 0, 0, 0), "D": (4, -1, 0, 0, 0)}
    for tok, w in want.items():
        for sname in D.SETTINGS:
            _, res, _ = run(D.Cell((tok,), dtype, sname, D.LAM[sname], 1.0, False, False))
            st = res["state"]
            assert (st["decision"][0], st["accepted_k"][0], st["fcalls"][0], st["rejects"][0], st["guards"][0]) == w, (tok, sname)
            assert st["consumed"][0] == 1 and st["null_tail"][0] == (tok == "Z")
            assert bool(st["flags"][0] & D.FLAG_NOT_FINITE) == (tok == "F")
            lam = dtype(D.LAM[sname])
            inc, dec = dtype(getattr(D.settings_of(dtype, D.SETTINGS[sname]), "lambdaIncrease")), dtype(getattr(D.settings_of(dtype, D.SETTINGS[sname]), "lambdaDecrease"))
            moved = {"A": dec * lam, "P": lam * inc, "R": lam * inc, "E": lam * inc, "I": lam * inc, "G": lam * inc, "Z": lam * inc}.get(tok, lam)
            assert st["lambda"][0] == moved and st["mu"][0] == (2 if tok in "PREIGZ" else 1), (tok, sname)


@pytest.mark.parametrize("dtype", DT)
def test_reject_and_rate_agree_with_the_shim(shim, dtype):  # noqa: F811
    from oracle import oracle as O
    suf, ct = ("d", C.c_double) if dtype == np.float64 else ("s", C.c_float)
    rng = np.random.default_rng(3)
    for sname, over in D.SETTINGS.items():
        So = O.default_settings(dtype)
        Sm = D.settings_of(dtype, over)
        for k, v in over.items():
            setattr(So, k, v)
        Sv = D.settings_values(Sm, dtype)
        assert all(dtype(getattr(So, k)) == Sv[k] for k in D.SETTING_FIELDS)
        lams = [dtype(v) for v in (1e-30, 1e-6, 1.5e-6, 0.125, 1.0, 37.7, 1e20)] + list((10.0 ** rng.uniform(-8, 8, 6)).astype(dtype))
        mus = [dtype(v) for v in (1, 2, 16, 128, D.MU_ODD, 1.3, 3.1)]
        rhos = [dtype(v) for v in (-1.0, 0.0, 0.05, 0.1, 0.2, 0.3, 0.5, 0.6, 0.8, 1.0, 7.0, np.inf)] \
            + [np.nextafter(Sv[k], dtype(d)) for k in ("minStepQuality", "goodStepQuality") for d in (0, 1)] + [Sv["minStepQuality"], Sv["goodStepQuality"]]
        for lam in lams:
            for mu in mus:
                l, m_ = ct(lam), ct(mu)
                getattr(shim, "lmr_reject_" + suf)(C.byref(l), C.byref(m_), So)
                with np.errstate(all="ignore"):
                    want = D.ref_reject(dtype, Sv, lam, mu)
                assert D.same_bits(np.array([l.value, m_.value], dtype=dtype), np.array(want, dtype=dtype)), (sname, lam, mu)
                for rho in rhos:
                    l, m_ = ct(lam), ct(mu)
                    getattr(shim, "lmr_rate_step_" + suf)(ct(rho), C.byref(l), C.byref(m_), So)
                    with np.errstate(all="ignore"):
                        want = D.ref_rate(dtype, Sv, rho, lam, mu)[:2]
                    assert D.same_bits(np.array([l.value, m_.value], dtype=dtype), np.array(want, dtype=dtype)), (sname, lam, mu, rho)


@pytest.mark.parametrize("name,dtype", D.REPLAY, ids=["%s-%s" % (n, np.dtype(d).name) for n, d in D.REPLAY])
def test_oracle_replay_through_the_reference(oracle, name, dtype):
    rejections, good = D.replay(D.walk, name, dtype)
    assert rejections >= 3 and good >= 1


def test_a_replay_without_rejections_fails(oracle, monkeypatch):
    real = D.oracle_rounds

    def only_acceptances(name, dtype):
        rounds, S = real(name, dtype)
        return [r for r in rounds if len(r["events"]) == 1 and r["events"][0][0] == 3 and r["mu"] == 1], S
    monkeypatch.setattr(D, "oracle_rounds", only_acceptances)
    with pytest.raises(AssertionError, match="nothing is shown"):
        D.replay(D.walk, "t3a", np.float64)


@pytest.mark.parametrize("plant", sorted(D.PLANTS))
def test_planted_mistake_fails_its_assertion(plant):
    cell, name = D.PLANTS[plant]
    _, good, _ = run(cell)
    _, bad, _ = run(cell, plant=plant)
    D.compare(good, good)
    with pytest.raises(AssertionError, match="^%s: " % name):
        D.compare(bad, good)


def test_a_moved_field_and_a_damaged_band_fail_by_name():
    cell = D.PLANTS["inf_error"][0]
    ops, good, path = run(cell)
    bad = dict(good, state=good["state"].copy())
    bad["state"]["rho"] = 1.0                                  # a rejection assigns no rho
    with pytest.raises(AssertionError, match="^rho: moved"):
        D.untouched(bad, ops, D.assigned_fields(path))
    with pytest.raises(AssertionError, match="^guard: "):
        D.compare(dict(good, guard=3), good)
    with pytest.raises(AssertionError, match="^rec: "):
        rec = good["rec"].copy()
        rec["reserved"][0] += 1
        D.compare(dict(good, rec=rec), good)


@pytest.mark.parametrize("dtype", DT)
def test_reduce32_reads_no_slot_behind_nparts_and_is_exact_on_integers(dtype):
    for nparts in D.NPARTS:
        ops = D.build(["R", "A"], dtype, 0.125, 1.0, nparts=nparts, seed=nparts)
        assert np.isnan(ops["partials"][:, nparts:]).all()
        assert [D.reduce32(ops["partials"][k], nparts) for k in range(2)] == [dtype(D.RESIDUAL + 20), dtype(D.RESIDUAL - 10)]


# ---------------------------------------------------------------------------------------------------------------- FD references
@pytest.mark.parametrize("dtype", DT)
def test_fd_points_reference_against_a_loop(dtype):
    kinds = set()
    for n in (1, 2, 7, 65):
        for bounds, shift, eps in (("inf", 0, F.EPS), ("finite", 0, F.EPS), ("finite", 4, F.EPS), ("finite", 1, F.EPS_LARGE)):
            x, lo, up = F.points_inputs(n, dtype, bounds, shift)
            for with_base in (False, True):
                a, b = F.points_reference(x, lo, up, eps, with_base), F.points_reference_slow(x, lo, up, eps, with_base)
                assert D.same_bits(a[0], b[0]) and D.same_bits(a[1], b[1]), (n, bounds, shift, eps)
            if bounds == "finite" and eps == F.EPS:
                _, twh = F.points_reference(x, lo, up, eps, False)
                kind = (np.arange(n) + shift) % 6
                kinds |= set(kind.tolist())
                assert np.all(twh[kind == 4] == 0) and np.all(twh[kind != 4] > 0)
                assert np.all(twh[(kind == 1) | (kind == 2)] == dtype(eps))
                near = (kind == 3) | (kind == 5)                # one side stops at eps / 2
                assert np.all((twh[near] > dtype(eps)) & (twh[near] < dtype(2 * eps)))
    assert kinds == set(range(6))


@pytest.mark.parametrize("dtype", DT)
def test_fd_fill_reference_against_a_loop(dtype):
    for m, n in ((1, 1), (5, 33), (9, 70)):
        for j0, pc in F.panels(n):
            Y, twh, J = F.fill_inputs(m, n, j0, pc, m + 3, dtype)
            assert D.same_bits(F.fill_reference(Y, twh, J, j0, pc), F.fill_reference_slow(Y, twh, J, j0, pc)), (m, n, j0, pc)
    assert F.panels(70) == [(0, 70), (0, 1), (5, 32), (33, 37), (69, 1)] and F.panels(1) == [(0, 1)] and F.panels(33) == [(0, 33), (0, 1), (32, 1)]
    Y, twh, J = F.fill_inputs(65, 33, 0, 33, 68, dtype, special=True)
    want = F.fill_reference(Y, twh, J, 0, 33)
    assert D.same_bits(want, F.fill_reference_slow(Y, twh, J, 0, 33)) and np.isinf(want).any() and np.isnan(want).any()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("m", F.STATE_MS)
def test_sum_of_squares_tree_stays_inside_the_bound(m, dtype):
    assert api.sumsq_blocks(m) == F.blocks_by_hand(m)
    v = F.random_vectors(m, dtype)[0]
    ref = F.fsum_squares(v)
    for order in ("kernel", "reversed", "pairwise"):
        err = abs(float(F.tree_sum_squares(v, order)) - ref) / ref
        assert err <= F.bound(m, dtype), (order, err, F.bound(m, dtype))
    e = F.exact_vectors(m, dtype)[0]
    assert float(F.tree_sum_squares(e)) == float((e.astype(np.int64) ** 2).sum())
    assert F.chain_length(131077) == 1 + 16 + 8 + 1 + 8 and F.chain_length(1) == 1 + 1 + 8 + 1 + 8


@pytest.mark.parametrize("dtype", DT)
def test_unpack_reference(dtype):
    for n in (1, 2, 5):
        for where in F.UNPACK_MAX:
            packed = F.unpack_inputs(n, dtype, where)
            JJ, Jy, jy_inf = F.unpack_reference(packed, n)
            assert np.array_equal(JJ, JJ.T) and len(set(np.tril(JJ)[np.tril_indices(n)].tolist())) == n * (n + 1) // 2
            assert all(JJ[i, j] == packed[i * (i + 1) // 2 + j] for i in range(n) for j in range(i + 1))
            assert jy_inf == (0 if where == "zero" else 1e6)
