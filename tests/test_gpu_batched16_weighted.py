"""Per-row weights and parameter covariance of the batched fit for models with 9 to 16 parameters, on the GPU
(k_lm_batched16<Model, true>, k_batched16_covariance<Model>: csrc/batched16_kernel.h; mir_optimize_least_squares_batched16_ex_d,
mir_lsq_batched16_kernel_ex_d, mir_lsq_batched16_covariance_d, launch_batched16<Model> with extras and
launch_batched16_covariance<Model>; M.optimizeLeastSquaresBatched16).

Problem sets: tests/batched16_weighted_problems.py (the families of tests/batched16_problems.py made heteroscedastic, w = 1 / sigma,
every fourth problem of the sets with m >= 130 with 37 zero weights). Fits are compared with the oracle minimising the WEIGHTED
objective (a Python f returning w (model - d); g = w J where the device uses grad) at the bar of tests/test_gpu_batched16.py,
its `compare`, imported: the same status class on every problem, every problem within the near bar (residual rtol 1e-7, x rtol
1e-3 / atol 1e-4), at most 5 % outside the tight one (1e-9, 1e-6 / 1e-7). The unweighted minimiser of every problem differs
from the weighted one beyond rtol 1e-6 (tests/test_batched16_weighted_host.py), so a fit that ignored its weights fails here.

Covariance: the reference is numpy float64 at the returned x, inv(J^T J) residual / dof from the analytic model Jacobian, dof
counted from the nonzero weights, compared entry-wise scaled by sd_i sd_j (weighted_problems.scaled_gap). Two bars, neither
taken from the code under test:
  finite differences   10 x the set's CPU covariance gap of float64 central differences at h = 2^-26 against the analytic
                       Jacobian (batched16_weighted_problems.CPU_FD_GAP, held to what the host test recomputes), rounded up to
                       one digit. The 10 is the margin of tests/test_gpu_batched_weighted.py: the device's exp / sin / cos and
                       its summation order.
  analytic             100 * 2^-52 * (the largest equilibrated condition number of the set's reference J^T J at the returned
                       x, computed here): a Cholesky inverse of a J^T J summed in another order, m <= 131 terms.
A wrong count of the degrees of freedom (m - n for a problem with 37 zero weights) moves the measure by 0.4 at m = 130 / 131:
five orders above either bar. Every comparison prints its worst gap before it asserts.
Measured on an MI355X, worst scaled gap over the 64 problems of a set (profiles/r15/batched16_weighted.txt holds the same figures):
  set                        Jacobian   weighted    abs. sigma  unweighted   bar (weighted | unweighted)
  EXP_HARM16  n = 16 m = 131   fd       2.031e-07   2.031e-07   1.422e-07    2e-06
  EXP_HARM16  n = 16 m = 131   grad     7.723e-12   7.728e-12   1.126e-13    4.7e-09 | 7.3e-11
  Harm<9>     n = 9  m = 67    fd       7.390e-08   7.390e-08   6.864e-08    6e-07
  Harm<9>     n = 9  m = 67    grad     3.271e-14   3.090e-14   2.384e-14    1.9e-11 | 1.2e-11
  Harm<13>    n = 13 m = 67    fd       1.419e-07   1.419e-07   1.460e-07    2e-06
  Harm<13>    n = 13 m = 67    grad     1.676e-13   1.722e-13   8.358e-14    7.0e-11 | 3.8e-11
  GAUSS3_AFFINE n = 11 m = 130 fd       6.555e-09   6.555e-09   5.326e-09    2e-07
"""
import ctypes as C
import functools

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import problems as P
import batched16_weighted_problems as WP16
from batched16_problems import COUNT, RDT
from test_gpu_batched16 import ANALYTIC, MAX_ROWS, Rec, boxed, compare, gaps

pytestmark = pytest.mark.gpu

ABSOLUTE_SIGMA = 1         # MIR_LSQ_BATCHED_ABSOLUTE_SIGMA


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def records(res):
    return [(int(r.status), r.iterations, r.fCalls, r.gCalls, np.float64(r.residual).tobytes(), np.float64(r.lambda_).tobytes()) for r in res]


def launch16(fn, x0, t, data, w=None, lo=None, up=None, variant=0, flags=0, cov=True, reps=1, model=None, cov_fn=None, rc_expected=0,
             recs=None):
    """An entry that takes extras on device data: mir_lsq_batched16_kernel_ex_d / mir_lsq_batched16_covariance_d (with `model`) or
    a user library's entry (without); the basis table is the call's own. Returns per launch (records, x, cov). With cov_fn (a
    covariance-only entry), its result on the LAST launch's device data is appended to the list. recs: the records on the
    device before the first launch (default: a pattern, so that a call that must touch nothing can be seen to)."""
    count, n = x0.shape
    m = data.shape[1]
    s = M.LeastSquaresSettings(np.float64)
    lo = np.full(n, -np.inf) if lo is None else lo
    up = np.full(n, np.inf) if up is None else up
    t_stride = 0 if t.ndim == 1 else m
    bufs = [api.DeviceBuffer(np.ascontiguousarray(a, dtype=np.float64)) for a in (t, data, x0, lo, up)]
    dt_, dd, dx, dlo, dup = bufs
    pattern = np.full(count * RDT.itemsize, 0x5A, np.uint8) if recs is None else np.ascontiguousarray(recs).view(np.uint8)
    dres = api.DeviceBuffer(pattern)
    dcov = api.DeviceBuffer(np.full((count, n, n), 7.0))
    dw = api.DeviceBuffer(np.ascontiguousarray(w, dtype=np.float64)) if w is not None else None
    st = api.Stream()
    opt = api.BatchedOptions(stream=st.handle, variant=variant)
    ex = api.BatchedExtras(flags=flags, weights=dw.ptr if dw else None, weight_stride=0 if (w is None or np.ndim(w) == 1) else m,
                           covariance=dcov.ptr if cov else None)
    head = [C.byref(s), count, m] + ([model] if model is not None else [])
    outs = []
    for _ in range(reps):
        dx.upload(np.ascontiguousarray(x0, dtype=np.float64))
        dcov.upload(np.full((count, n, n), 7.0))
        rc = fn(*head, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr, dres.ptr, C.byref(opt), C.byref(ex))
        assert rc == rc_expected, rc
        st.synchronize()
        outs.append((np.frombuffer(dres.download().tobytes(), dtype=RDT).copy(), dx.download().reshape(count, n).copy(),
                     dcov.download().reshape(count, n, n).copy()))
    if cov_fn is not None:
        dcov.upload(np.full((count, n, n), 7.0))
        rc = cov_fn(*head, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr, dres.ptr, C.byref(opt), C.byref(ex))
        assert rc == 0, rc
        st.synchronize()
        outs.append(dcov.download().reshape(count, n, n).copy())
    for b in bufs + [dres, dcov] + ([dw] if dw else []):
        b.free()
    return outs


@functools.lru_cache(maxsize=None)
def user_lib():
    UL = C.CDLL(hipbuild.user_model_n16_weighted_lib())
    for n in (9, 13):
        for name in (f"user_fit_weighted_harm{n}_d", f"user_weighted_harm{n}_covariance_d"):
            fn = getattr(UL, name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 4
    return UL


def kernel_ex():
    return api.lib().mir_lsq_batched16_kernel_ex_d


def fit_set(key, w="set", variant=0, flags=0, cov=True, cov_only=False):
    """the set's fit on the device: the built-in models through the host entry (M.optimizeLeastSquaresBatched16), n = 9 and 13
    through the caller's library on device data. w: "set" (the set's weights), None, or an array. Returns (res, x, cov) and, with
    cov_only, the covariance-only entry's result on the same device data"""
    family, n, m = key
    t, data, x0, ws = WP16.model_of(key)[:4]
    w = ws if isinstance(w, str) else w
    if family == "harm" and n != 16:
        UL = user_lib()
        out = launch16(getattr(UL, f"user_fit_weighted_harm{n}_d"), x0, t, data, w, variant=variant, flags=flags, cov=cov,
                       cov_fn=getattr(UL, f"user_weighted_harm{n}_covariance_d") if cov_only else None)
        raw, x, cv = out[0]
        return ([Rec(r) for r in raw], x, cv) + ((out[1],) if cov_only else ())
    model = M.MODEL16_EXP_HARM16 if family == "harm" else M.MODEL16_GAUSS3_AFFINE
    if cov_only:
        out = launch16(kernel_ex(), x0, t, data, w, variant=variant, flags=flags, model=model, cov_fn=api.lib().mir_lsq_batched16_covariance_d)
        raw, x, cv = out[0]
        return [Rec(r) for r in raw], x, cv, out[1]
    out = M.optimizeLeastSquaresBatched16(model, x0, t, data, variant=variant, weights=w, covariance=cov,
                                          absolute_sigma=bool(flags & ABSOLUTE_SIGMA))
    return out if cov else out + (None,)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("harm", 16, 131), ("gauss3", 11, 130)], ids=["harm16-m131", "gauss3-m130"])
def test_weights_of_ones_give_the_bits_of_the_unweighted_fit_of_the_old_entry(key):
    t, data, x0, w = WP16.model_of(key)[:4]
    model = M.MODEL16_EXP_HARM16 if key[0] == "harm" else M.MODEL16_GAUSS3_AFFINE
    res0, xa = M.optimizeLeastSquaresBatched(model, x0, t, data, dtype=np.float64)                 # mir_optimize_least_squares_batched16_d
    res1, xb = M.optimizeLeastSquaresBatched16(model, x0, t, data, weights=np.ones(t.size))
    res2, xc = M.optimizeLeastSquaresBatched16(model, x0, t, data, weights=np.ones_like(w))
    assert (bits(xa) == bits(xb)).all() and (bits(xa) == bits(xc)).all()
    assert records(res0) == records(res1) == records(res2)
    assert sum(r.iterations for r in res0) > 3 * COUNT and all(r.status >= 0 for r in res0)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
FIT_CASES = [(("harm", 16, 33), 0), (("harm", 16, 33), ANALYTIC), (("harm", 16, 67), 0), (("harm", 16, 67), ANALYTIC),
             (("harm", 16, 131), 0), (("harm", 16, 131), ANALYTIC), (("harm", 9, 67), 0), (("harm", 9, 67), ANALYTIC),
             (("harm", 13, 67), 0), (("harm", 13, 67), ANALYTIC), (("gauss3", 11, 130), 0)]


@pytest.mark.parametrize("key,variant", FIT_CASES, ids=[f"{k[0]}{k[1]}-m{k[2]}-{'analytic' if v else 'fd'}" for k, v in FIT_CASES])
def test_weighted_fits_match_the_oracle_on_the_weighted_objective(oracle, key, variant):
    res, x, _ = fit_set(key, variant=variant, cov=False)
    ref = WP16.oracle_fits(oracle, key, analytic=bool(variant))
    assert all(ro.status >= 0 for ro, _ in ref)
    assert all(r.iterations >= 1 for r in res) and all((r.gCalls >= 1) == bool(variant) for r in res)
    compare(res, x, ref)                                                    # also: no status -100


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_zero_weights_equal_shorter_problems():
    """Rows of weight 0, filled with garbage data, against the truncated problems launched on their own at the smaller m. Every
    zero-weight row contributes exact zeros to every sum, so the two fits are expected to agree bit for bit (printed); the
    assertion is the parity bar."""
    n, m = 16, 131
    t, B, data, x0, w = WP16.harm_weighted(n, m, zero="tail")
    sel = slice(0, COUNT, 4)                                                # the problems with the 37 zero weights
    data, x0, w = data[sel], x0[sel], w[sel]
    ms = m - WP16.ZERO_TAIL
    assert ms == 94 and (w[:, ms:] == 0).all() and (w[:, :ms] != 0).all()
    garbage = data.copy()
    u = P.splitmix64_uniform(4242, data.shape[0] * WP16.ZERO_TAIL).reshape(-1, WP16.ZERO_TAIL)
    garbage[:, ms:] = 1e3 * (u - 0.5)
    res_a, xa = M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x0, t, garbage, weights=w)
    res_b, xb = M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x0, t[:ms], data[:, :ms], weights=w[:, :ms])
    same = (bits(xa) == bits(xb)).all() and records(res_a) == records(res_b)
    print(f"zero weights against truncation, n = 16, m = 131 -> 94: bit-identical = {same}")
    # (no status is asserted: 94 rows on t <= 2.87 leave the 13 harmonics of period 4 / k a J^T J of condition 1e12, on which the
    # oracle too runs into maxIterations on half of these problems; the comparison is the kernel's with itself)
    assert all(r.iterations >= 1 for r in res_a)
    compare(res_a, xa, list(zip(res_b, xb)))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_shared_weights_give_the_bits_of_tiled_ones():
    key = ("harm", 16, 67)
    t, data, x0, w = WP16.model_of(key)[:4]
    fit = lambda ww, **kw: M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x0, t, data, weights=ww, **kw)
    res0, xa, ca = fit(w[1], covariance=True)
    res1, xb, cb = fit(np.tile(w[1], (COUNT, 1)), covariance=True)
    assert (bits(xa) == bits(xb)).all() and records(res0) == records(res1) and (bits(ca) == bits(cb)).all()
    assert np.isfinite(ca).all()
    w2 = np.tile(w[1], (COUNT, 1)); w2[7] *= 1.5                            # problem 7 sees other weights
    res2, xc, cc = fit(w2, covariance=True)
    same = (bits(xa) == bits(xc)).all(axis=1)
    assert same[np.arange(COUNT) != 7].all() and not same[7]
    same_cov = (bits(ca) == bits(cc)).reshape(COUNT, -1).all(axis=1)
    assert same_cov[np.arange(COUNT) != 7].all() and not same_cov[7]


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_bounded_and_weighted(oracle):
    """the bounded set of test_gpu_batched16 (p3 .. p15 boxed to +- 0.25, the start clipped into the box) with the weighted data
    of this file, against the oracle with the same box on the weighted objective, as that test compares: the residual to rtol
    1e-6 on every problem, the problems on which the oracle's own two summation orders disagree set aside (at most 10 %), the
    rest at the parity bar"""
    n, m = 16, 67
    key = ("harm", n, m)
    t, data, x0, w = WP16.model_of(key)[:4]
    _, _, _, lo, up, starts = boxed(n, m)
    res, x, cov = M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, starts, t, data, l=lo, u=up, weights=w, covariance=True)
    ref = WP16.oracle_fits(oracle, key, box=(lo, up, starts))
    again = WP16.oracle_fits(oracle, key, box=(lo, up, starts), reverse=True)
    on_bound = [int(np.sum((xr == lo) | (xr == up))) for _, xr in ref]
    assert sum(1 for c in on_bound if c >= 1) >= COUNT // 2, on_bound      # the box binds on most problems
    assert all(r.status >= 0 for r in res), [int(r.status) for r in res]
    assert np.isfinite(cov).all() and (bits(cov) == bits(cov.transpose(0, 2, 1))).all()
    aside = set()
    for k, ((rr, xr), (r2, x2)) in enumerate(zip(ref, again)):
        assert rr.status >= 0, (k, rr.status)
        assert np.all(x[k] >= lo) and np.all(x[k] <= up), k                # inside the box exactly
        assert abs(res[k].residual / rr.residual - 1) <= 1e-6, (k, res[k].residual, rr.residual)
        if not gaps(r2, x2, rr, xr)[0]:
            aside.add(k)
    print(f"set aside {sorted(aside)}; parameters on a bound {on_bound}")
    assert len(aside) <= 0.10 * COUNT, sorted(aside)
    compare(res, x, ref, skip=aside)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def covariance_gaps(key, w, x, cov, res, absolute_sigma=False):
    """(worst scaled gap of `cov` against the numpy float64 reference at the returned x, largest equilibrated condition number)"""
    t, data, _, _, value, jac = WP16.model_of(key)
    worst = cond = 0.0
    for k in range(x.shape[0]):
        wk = np.asarray(w if np.ndim(w) == 1 else w[k], dtype=np.float64)
        r = wk * (value(x[k]) - data[k])
        assert np.isclose(r @ r, res[k].residual, rtol=1e-9), (k, r @ r, res[k].residual)       # the record's residual is ||w f(x)||^2
        J = jac(x[k])
        ref = WP16.reference_covariance(J, wk, r @ r, absolute_sigma)
        assert np.all(np.isfinite(cov[k])), (k, cov[k])
        assert (bits(cov[k]) == bits(cov[k].T.copy())).all(), k              # symmetric, bit for bit
        worst = max(worst, WP16.scaled_gap(cov[k], ref))
        cond = max(cond, WP16.equilibrated_cond(J * wk[:, None]))
    return worst, cond


COV_CASES = [(("harm", 16, 131), 0), (("harm", 16, 131), ANALYTIC), (("harm", 9, 67), 0), (("harm", 9, 67), ANALYTIC),
             (("harm", 13, 67), 0), (("harm", 13, 67), ANALYTIC), (("gauss3", 11, 130), 0)]


@pytest.mark.parametrize("key,variant", COV_CASES, ids=[f"{k[0]}{k[1]}-m{k[2]}-{'analytic' if v else 'fd'}" for k, v in COV_CASES])
def test_covariance_against_numpy_at_the_returned_x(key, variant):
    """with and without ABSOLUTE_SIGMA, weighted and unweighted; the problems with 37 zero weights use dof = m - 37 - n (the
    reference counts the nonzero weights)"""
    t, data, x0, w = WP16.model_of(key)[:4]
    res, x, cov = fit_set(key, variant=variant)
    assert all(r.status >= 0 for r in res)
    gap, cond = covariance_gaps(key, w, x, cov, res)
    res_a, xa, cova = fit_set(key, variant=variant, flags=ABSOLUTE_SIGMA)
    assert (bits(xa) == bits(x)).all()
    gap_abs, _ = covariance_gaps(key, w, xa, cova, res_a, absolute_sigma=True)
    ones = np.ones(t.size)
    res_u, xu, covu = fit_set(key, w=None, variant=variant)                  # unweighted: dof = m - n
    assert all(r.status >= 0 for r in res_u)
    gap_u, cond_u = covariance_gaps(key, ones, xu, covu, res_u)
    if variant:
        bar, bar_u = 100 * 2.0 ** -52 * cond, 100 * 2.0 ** -52 * cond_u
    else:
        bar = bar_u = WP16.fd_bar(key)
    print(f"covariance {key} {'analytic' if variant else 'fd'}: worst scaled gap weighted {gap:.3e}, absolute sigma {gap_abs:.3e} "
          f"(bar {bar:.1e}; cond {cond:.2e}), unweighted {gap_u:.3e} (bar {bar_u:.1e}; cond {cond_u:.2e})")
    assert gap <= bar and gap_abs <= bar and gap_u <= bar_u, (gap, gap_abs, bar, gap_u, bar_u)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,variant", [(("harm", 16, 131), 0), (("gauss3", 11, 130), 0), (("harm", 9, 67), ANALYTIC), (("harm", 13, 67), 0)],
                         ids=["harm16", "gauss3", "user9-analytic", "user13-fd"])
def test_the_covariance_entry_reproduces_the_covariance_of_the_fit_launch(key, variant):
    res, x, cov, cov2 = fit_set(key, variant=variant, cov_only=True)
    assert all(r.status >= 0 for r in res) and np.isfinite(cov).all()
    assert (bits(cov) == bits(cov2)).all()


def test_degenerate_covariance():
    """+inf: (a) no degrees of freedom -- all but 16 weights zero at n = 16 on the even problems, through the whole fit where
    that fit ends with a status >= 0, and through the covariance entry on hand-made records for every one of them; (b) a J^T J
    that is singular EXACTLY -- EXP_HARM16 at an x with x[0] = 0, so that the column of the rate is zero in every row, by
    finite differences and by grad. NaN: a problem whose start holds a NaN (status -31); its neighbours are not affected."""
    n, m, count = 16, 131, 16
    t, B, data, x0, w = WP16.harm_weighted(n, m)
    data, x0, w = data[:count], np.array(x0[:count]), w[:count]
    keep = np.arange(3, m, 8)[:16]
    w16 = np.zeros_like(w); w16[:, keep] = np.where(w[:, keep] != 0, w[:, keep], 1.0)
    w16[1::2] = w[1::2]                                                     # odd problems keep all their rows
    assert (np.count_nonzero(w16[0::2], axis=1) == 16).all()
    x0[5, 2] = np.nan
    res, x, cov = M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x0, t, data, weights=w16, covariance=True)
    print("statuses with 16 rows left on the even problems:", [int(r.status) for r in res])
    assert int(res[5].status) == -31 and np.isnan(cov[5]).all()
    for k in range(count):
        if k == 5:
            continue
        if k % 2:
            assert res[k].status >= 0, (k, int(res[k].status))
            assert np.isfinite(cov[k]).all() and (np.diag(cov[k]) > 0).all(), (k, cov[k])
        elif res[k].status >= 0:
            assert (cov[k] == np.inf).all(), (k, cov[k])
        else:
            assert np.isnan(cov[k]).all(), (k, cov[k])
    # hand-made records (status 1, residual 1): the covariance entry alone
    recs = np.zeros(count, dtype=RDT); recs["status"] = 1; recs["residual"] = 1.0
    xs = np.tile(np.concatenate([[1.0, 2.0, 0.1], np.linspace(-0.3, 0.3, 13)]), (count, 1))
    covfn = api.lib().mir_lsq_batched16_covariance_d
    for variant in (0, ANALYTIC):
        (_, _, out), = launch16(covfn, xs, t, data, w16, variant=variant, model=M.MODEL16_EXP_HARM16, recs=recs)
        assert (out[0::2] == np.inf).all(), variant                         # (a): 16 rows, 16 parameters
        assert np.isfinite(out[1::2]).all(), variant
        xz = xs.copy(); xz[0::2, 0] = 0.0                                   # (b)
        (_, _, out), = launch16(covfn, xz, t, data, w, variant=variant, model=M.MODEL16_EXP_HARM16, recs=recs)
        assert (out[0::2] == np.inf).all(), (variant, out[0])
        assert np.isfinite(out[1::2]).all(), variant                        # a non-negative status never gives NaN


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_two_identical_weighted_launches_on_device_data_are_bit_identical():
    t, data, x0, w = WP16.model_of(("harm", 16, 67))[:4]
    (r1, x1, c1), (r2, x2, c2) = launch16(kernel_ex(), x0, t, data, w, model=M.MODEL16_EXP_HARM16, reps=2)
    assert r1.tobytes() == r2.tobytes() and x1.tobytes() == x2.tobytes() and c1.tobytes() == c2.tobytes()
    assert np.all(r1["status"] >= 0) and r1["iterations"].sum() > 3 * COUNT and np.isfinite(c1).all()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_the_row_limit(oracle):
    n, count = 16, 8
    t, B, data, x0, w = WP16.harm_weighted(n, MAX_ROWS, count)
    assert (np.count_nonzero(w == 0, axis=1)[[0, 4]] == WP16.ZERO_TAIL).all()
    res, x, cov = M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x0, t, data, weights=w, covariance=True)     # return code 0
    ref = WP16.oracle_fits(oracle, ("harm", n, MAX_ROWS), count=count)
    assert all(ro.status >= 0 for ro, _ in ref)
    compare(res, x, ref)
    assert np.isfinite(cov).all() and (bits(cov) == bits(cov.transpose(0, 2, 1))).all() and (np.einsum("kii->ki", cov) > 0).all()
    # one row more: -3 from every entry, and nothing is touched
    t1, B1, d1, x1, w1 = WP16.harm_weighted(n, MAX_ROWS + 1, count)
    with pytest.raises(RuntimeError, match="-3"):
        M.optimizeLeastSquaresBatched16(M.MODEL16_EXP_HARM16, x1, t1, d1, weights=w1, covariance=True)
    for fn in (kernel_ex(), api.lib().mir_lsq_batched16_covariance_d):
        (raw, xo, co), = launch16(fn, x1, t1, d1, w1, model=M.MODEL16_EXP_HARM16, rc_expected=-3)
        assert raw.tobytes() == bytes([0x5A]) * (count * RDT.itemsize) and (bits(xo) == bits(np.array(x1))).all() and (co == 7.0).all()
