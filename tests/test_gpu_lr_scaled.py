"""J0 kept as the unscaled finite-difference difference panel: the fused FD kernel of a refresh does not
write J, the Broyden sweeps and the flush read the panel and scale what they load. Every comparison here is BITWISE.

  kernels   the scaled pass (mir_lsq_lr_pass_scaled_d) against the plain pass on the J that mir_lsq_fd_diff_jtj_d writes from the
            same panel and widths, and the scaled flush against the plain flush of that J: tests/lr_scaled_cases.py has the cells
            (every scaled instance: tests/test_lr_scaled_cell_coverage.py), the data and what is compared.
  solves    the default path against MIR_LSQ_VARIANT_FD_WRITE_J, the restatement that writes J on every refresh: x, residual,
            status, iterations, fCalls, every counter of the statistics -- through flushes while J0 is in the panel, several
            refreshes, the one-by-one rounds, the entry residual by a call of its own, row shards, covariance() and a reused
            workspace."""
import ctypes as C
import threading

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, workloads as W
import lr_cases as LC
import lr_scaled_cases as S
import problems as P

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- kernels
_refs = {}


def reference(m, n, off, poisoned):
    """(panel, twh, J) of a shape, formed once and shared by the cells of that shape (nobody writes to them)"""
    key = (m, n, off, poisoned)
    if key not in _refs:
        D, twh = S.panel_case(m, n, poisoned)
        y = np.zeros(m)
        J = S.reference_J(D, twh, y, off)
        for a in (D, twh, J):
            a.setflags(write=False)
        _refs[key] = (D, twh, J)
    return _refs[key]


@pytest.mark.parametrize("n", S.NS)
def test_scaled_pass_has_the_bits_of_the_plain_pass(n):
    ran = 0
    for c in (c for c in S.CELLS if c.kind == "pass" and c.n == n):
        D, twh, J = reference(c.m, n, c.off, c.poisoned)
        inp = S.pass_inputs(c.m, n, c.k, seed=1 + c.off)
        plain = LC.run_pass(LC.Cell("pass", np.float64, c.m, n, c.k, c.off, c.mode, 1), dict(inp, J=J))
        scaled = S.run_pass_scaled(c, D, twh, inp)
        try:
            S.check_same_pass(scaled, plain, finished=c.mode == "plain")
            if c.mode == S.NOGO:
                LC.check_nogo(scaled, dict(inp, J=J))                    # the sum of squares only, zeros for the rest
            elif not c.poisoned:
                assert np.all(np.isfinite(scaled["reduced"])) and np.all(np.isfinite(scaled["U_col"])), "a collapsed column's NaN / Inf got through"
            else:
                assert not np.all(np.isfinite(scaled["reduced"])), "the live column's NaN did not propagate"
        except AssertionError as e:
            raise AssertionError(f"{c}: {e}") from None
        ran += 1
    assert ran == len(S.MS) * len(S.offsets(n)) * (len(S.SWEEP_KS) + 2 + int(S.has_live_column(n)))


@pytest.mark.parametrize("n", S.NS)
def test_scaled_flush_materialises_the_plain_flush_of_J(n):
    ran = 0
    for c in (c for c in S.CELLS if c.kind == "flush" and c.n == n):
        D, twh, J = reference(c.m, n, c.off, False)
        inp = S.pass_inputs(c.m, n, c.k, seed=3 + c.off)
        fin = dict(J=J, U=inp["U"], D=inp["D"])
        want = LC.run_flush(LC.Cell("flush", np.float64, c.m, n, c.k, c.off, "", 0), fin)
        got = S.run_flush_scaled(c, D, twh, fin)                         # (asserts the panel unchanged between its guard bands)
        bad = np.argwhere(S.bits(got) != S.bits(want))
        assert bad.size == 0, f"{c}: flushed J differs at {bad[:4].tolist()}"
        assert np.all(np.isfinite(got)), f"{c}: a collapsed column's NaN / Inf got through"
        ran += 1
    assert ran == len(S.MS) * len(S.offsets(n)) * len(S.FLUSH_KS)


def test_fd_kernel_without_a_J_forms_the_same_products():
    """mir_lsq_fd_diff_jtj_d with J = NULL: JJ and Jy have the bits of the call that writes J"""
    for m, n in ((515, 16), (2050, 128), (300, 100), (259, 192), (130, 256)):
        D, twh = S.panel_case(m, n, False)
        y = np.random.default_rng(n).standard_normal(m)
        _, JJ1, Jy1, _ = api.fd_jtj(D, twh, y, diff=True)
        J0, JJ0, Jy0, _ = api.fd_jtj(D, twh, y, diff=True, write_J=False)
        assert J0 is None and np.array_equal(S.bits(JJ0), S.bits(JJ1)) and np.array_equal(S.bits(Jy0), S.bits(Jy1)), (m, n)


# ---------------------------------------------------------------- whole solves
COUNTERS = [k for k, t in M.Stats._fields_ if t is C.c_uint64 or (isinstance(t, type) and issubclass(t, C.Array) and t._type_ is C.c_uint64)]


def outcome(r, x, st):
    d = st.as_dict()
    return (x.tobytes(), np.float64(r.residual).tobytes(), int(r.status), r.iterations, r.fCalls, r.gCalls, np.float64(r.lambda_).tobytes(),
            tuple((k, tuple(d[k]) if isinstance(d[k], list) else d[k]) for k in COUNTERS))


def both(prob, x0, lo=None, up=None, settings=None, extra=0, **kw):
    """the same solve on the default path and with the J write restored: ([outcome, outcome], [stats, stats])"""
    outs, stats = [], []
    for variant in (0, M.VARIANT_FD_WRITE_J):
        st = M.Stats()
        r, x = prob.solve(x0, l=lo, u=up, settings=settings, stats=st, variant=variant | extra, batched=True, **kw)
        outs.append(outcome(r, x, st))
        stats.append(st)
    return outs, stats


def settings(tol=1e-9, **kw):
    s = M.LeastSquaresSettings()
    s.absTolerance = tol
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def same(outs):
    assert outs[0][:7] == outs[1][:7], [o[2:6] for o in outs]
    assert outs[0][7] == outs[1][7], [kv for kv, kw in zip(outs[0][7], outs[1][7]) if kv != kw]


@pytest.mark.parametrize("m,n", [(2050, 128), (515, 16), (1030, 192), (1031, 256), (1030, 100)])
def test_default_path_has_the_bits_of_the_path_that_writes_J(m, n):
    w = P.tanh_linear(m, n)
    prob = W.TanhLinear(w["A"], w["b"])
    outs, stats = both(prob, w["x0"], settings=settings())
    same(outs)
    assert outs[0][2] >= 0 and stats[0].jacobian_full >= 1 and stats[0].jacobian_broyden >= 2 and stats[0].fd_callback_calls >= 1


@pytest.mark.parametrize("m,n", [(2050, 128), (515, 16)])
def test_bounds_that_collapse_an_interval(m, n):
    """lower = upper = x0 in one parameter: twh = 0 there, a zero column of J (LS:1046) in every refresh"""
    w = P.tanh_linear(m, n)
    prob = W.TanhLinear(w["A"], w["b"])
    lo, up = np.full(n, -np.inf), np.full(n, np.inf)
    lo[3] = up[3] = w["x0"][3]
    lo[n - 1] = w["xstar"][n - 1] + 0.02                                 # and one bound the minimiser violates
    x0 = np.maximum(w["x0"], np.where(np.isfinite(lo), lo, -np.inf))
    outs, stats = both(prob, x0, lo, up, settings())
    same(outs)
    assert outs[0][2] >= 0 and stats[0].jacobian_broyden >= 2


@pytest.mark.parametrize("m,n", [(2050, 128), (515, 16), (1030, 192), (1031, 256)])
def test_flush_and_resynchronisation_while_J0_is_in_the_panel(m, n):
    """two pending terms at most (bits 16..20): the flush materialises J from the panel, J^T J is recomputed from it, and the
    passes behind it sweep J itself"""
    w = P.tanh_linear(m, n)
    prob = W.TanhLinear(w["A"], w["b"])
    outs, stats = both(prob, w["x0"], settings=settings(1e-10), extra=M.variant_lr_cap(2))
    same(outs)
    st = stats[0]
    assert st.broyden_flushes >= 1 and st.jtj_resyncs == st.broyden_flushes and st.jacobian_broyden >= 4, st.as_dict()


@pytest.mark.parametrize("m,n", [(2050, 128), (515, 16)])
def test_three_refreshes(m, n):
    w = P.tanh_linear(m, n)
    prob = W.TanhLinear(w["A"], w["b"])
    outs, stats = both(prob, w["x0"], settings=settings(1e-10, maxAge=2))
    same(outs)
    assert stats[0].jacobian_full >= 3 and stats[0].jacobian_broyden >= 2
    outs, stats = both(prob, w["x0"], settings=settings(1e-10, maxAge=2), extra=M.variant_lr_cap(1))      # a flush between two refreshes
    same(outs)
    assert stats[0].jacobian_full >= 3 and stats[0].broyden_flushes >= 1


@pytest.mark.parametrize("extra", [M.VARIANT_NO_PIPELINE, M.VARIANT_NO_FD_BASE_POINT, M.VARIANT_NO_PIPELINE | M.VARIANT_NO_FD_BASE_POINT],
                         ids=["one-by-one", "no-base-point", "both"])
def test_one_by_one_rounds_and_the_entry_residual_by_its_own_call(extra):
    for m, n in ((2050, 128), (515, 16)):
        w = P.tanh_linear(m, n)
        prob = W.TanhLinear(w["A"], w["b"])
        outs, stats = both(prob, w["x0"], settings=settings(), extra=extra)
        same(outs)
        assert stats[0].jacobian_broyden >= 2 and (stats[0].fused_rounds == 0) == bool(extra & M.VARIANT_NO_PIPELINE)
        ref, _ = both(prob, w["x0"], settings=settings())
        assert outs[0][:7] == ref[0][:7]                                 # and the bits of the default flow


def test_two_row_shards():
    from mir_optim_amd import parallel as PAR
    m_total, n, world = 2050, 128, 2
    s = settings()
    full = P.tanh_linear(m_total, n)
    probs = []
    for r in range(world):
        off, ml = PAR.row_shard(m_total, world, r)
        w = P.tanh_linear(ml, n, row_offset=off, m_total=m_total)
        probs.append(W.TanhLinear(w["A"], w["b"]))
    per_variant = []
    for variant in (0, M.VARIANT_FD_WRITE_J):
        comms, close = PAR.local_group(world)
        res, err, sts = [None] * world, [None] * world, [M.Stats() for _ in range(world)]

        def one(r):
            try:
                rr, xx = probs[r].solve(full["x0"], settings=s, comm=comms[r], stats=sts[r], batched=True, variant=variant)
                res[r] = outcome(rr, xx, sts[r])
            except BaseException as e:   # noqa: BLE001
                err[r] = e
        ts = [threading.Thread(target=one, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(600)
        close()
        assert not any(t.is_alive() for t in ts) and not any(err), err
        assert len({o[:7] for o in res}) == 1                            # every rank: the same bits
        per_variant.append(res)
    for r in range(world):
        same([per_variant[0][r], per_variant[1][r]])
    assert sts[0].jacobian_broyden >= 2


def test_covariance_and_a_second_solve_on_the_same_workspace():
    """covariance() makes a refresh of its own on the solve's workspace (panel and widths replaced, no sweep behind it), and the next
    solve on that workspace starts from a refresh again: the bits of solves that own their workspace, with either variant"""
    m, n = 2050, 128
    w = P.tanh_linear(m, n)
    prob = W.TanhLinear(w["A"], w["b"])
    s = settings()
    fresh, _ = both(prob, w["x0"], settings=s)
    same(fresh)
    covs = []
    for variant in (0, M.VARIANT_FD_WRITE_J):
        ws = api.lib().mir_lsq_workspace_create(m, n, 8)
        assert ws
        try:
            runs = []
            for _ in range(2):                                           # two solves back to back
                st = M.Stats()
                r, x = prob.solve(w["x0"], settings=s, stats=st, batched=True, workspace=ws, variant=variant)
                runs.append(outcome(r, x, st))
            opts = prob.options(batched=True, workspace=ws, variant=variant)
            cov, _, res, info = M.covariance(prob.f, prob.m, x, options=opts, fContext=C.addressof(prob.ctx))
            assert info == 0
            covs.append((cov.tobytes(), np.float64(res).tobytes()))
            st = M.Stats()
            r, x = prob.solve(w["x0"], settings=s, stats=st, batched=True, workspace=ws, variant=variant)
            runs.append(outcome(r, x, st))
        finally:
            api.lib().mir_lsq_workspace_destroy(ws)
        for o in runs:
            same([o, fresh[0]])
    assert covs[0] == covs[1]
