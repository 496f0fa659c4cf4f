"""Per-problem bounds (MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM: lower / upper hold count x n values, row k the box of problem k)
and fixed parameters (l_j == u_j) on the batched one-wavefront-per-problem fits, on the GPU: k_lm_batched (default and bounded
instance, float and double, weighted and not), k_lm_batched16, k_batched_covariance and k_batched16_covariance, through the
kernel entries, the host entries, the covariance entries and the public device header.

Families, launchers, references and the restated parity bars: tests/problem_bounds_cases.py. The structural tests compare BITS.
The covariance reference is numpy float64 on the FREE columns (analytic Jacobian at the returned x, s^2 = residual / (rows -
n_free), zeros in the rows and columns of the fixed parameters), compared on the free block scaled by sd_i sd_j at the bars of
the existing covariance tests for the same model, precision and Jacobian kind (tests/test_gpu_batched_weighted.py COV_BAR;
tests/test_gpu_batched16_weighted.py: 10 x the CPU's own finite-difference gap for central differences, 100 * 2^-52 * cond
for the analytic Jacobian). Every comparison prints its figures before it asserts."""
import numpy as np
import pytest

import mir_optim_amd as M
import problems as P
import batched16_weighted_problems as WP16
import problem_bounds_cases as PB

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SMALL = [pytest.param(name, dtype, id=f"{name}-{np.dtype(dtype).name}") for name in ("PB3", "PB8") for dtype in (F32, F64)]
WIDE = ["PB16h", "PB16h9", "PB16g"]
ALL = SMALL + [pytest.param(name, F64, id=name) for name in WIDE]
# the covariance bars of the existing tests, by (family, precision) for central differences
FD_BAR = {("PB3", F64): 7e-8, ("PB8", F64): 2e-6, ("PB3", F32): 2e-3, ("PB8", F32): 4e-1,
          ("PB16h", F64): WP16.fd_bar(("harm", 16, 67)), ("PB16h9", F64): WP16.fd_bar(("harm", 9, 67)),
          ("PB16g", F64): WP16.fd_bar(("gauss3", 11, 130))}


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def variants_of(fam, instance):
    """the variant words a family is launched with: the n <= 8 families by instance (default / DEVICE_BOUNDS), the 16-lane
    kernel by Jacobian kind where the model has grad"""
    if not fam.wide:
        return [PB.DEVICE_BOUNDS if instance == "bounded" else 0]
    return [0, PB.ANALYTIC] if fam.has_grad else [0]


# ------------------------------------------------------------------------------------------------------------ 1: bit identity
@pytest.mark.parametrize("instance", ["default", "bounded"])
@pytest.mark.parametrize("name, dtype", SMALL)
def test_every_problem_has_the_bits_of_its_own_shared_bounds_launch(name, dtype, instance):
    """Problem k of ONE per-problem-bounds launch has the records and x, bit for bit, of a shared-bounds launch of that problem
    alone with row k as its box: unweighted and with weights that end in a zero-weight tail, with shared and with per-problem
    abscissae. The default instance: -100 is part of the record."""
    fam = PB.family(name)
    variant, = variants_of(fam, instance)
    for w in (None, PB.weights_for(fam)):
        for own_t in (False, True):
            raw, x, _ = PB.fit_family(fam, dtype, variant=variant, w=w, own_t=own_t)
            assert np.all((raw["status"] >= 0) | (raw["status"] == -100)), raw["status"]
            if instance == "bounded":
                assert np.all(raw["status"] >= 0) and raw["iterations"].sum() > fam.count
            else:
                assert np.any(raw["status"] == -100)              # PB8: every problem, at its first step
            for k in range(fam.count):
                one = PB.fit_one(fam, k, dtype, variant=variant, w=w, own_t=own_t)
                assert one[0].tobytes() == raw[k:k + 1].tobytes() and one[1].tobytes() == x[k:k + 1].tobytes(), (k, own_t, one[0], raw[k])


@pytest.mark.parametrize("name", WIDE)
def test_every_problem_of_the_16_lane_kernel_has_the_bits_of_its_own_shared_bounds_launch(name):
    """k_lm_batched16, unweighted and weighted, finite differences and (where the model has grad) ANALYTIC_JACOBIAN, shared and
    per-problem abscissae; the built-in models also through the entry without _ex (an extras that carries the flag alone)"""
    fam = PB.family(name)
    for variant in variants_of(fam, None):
        for w in (None, PB.weights_for(fam)):
            for own_t in (False, True):
                raw, x, _ = PB.fit_family(fam, F64, variant=variant, w=w, own_t=own_t)
                # -26: weighted PB16h, problem 8 -- a box QP that does not end as solved; the oracle ends that fit the same way
                assert np.all((raw["status"] >= 0) | (raw["status"] == -26)) and np.sum(raw["status"] < 0) <= 1, raw["status"]
                assert raw["iterations"].sum() > fam.count
                for k in range(fam.count):
                    one = PB.fit_one(fam, k, F64, variant=variant, w=w, own_t=own_t)
                    assert one[0].tobytes() == raw[k:k + 1].tobytes() and one[1].tobytes() == x[k:k + 1].tobytes(), (k, variant, own_t)
        if fam.model is not None:
            assert same(PB.fit_family(fam, F64, variant=variant, plain16=True), PB.fit_family(fam, F64, variant=variant))


# ------------------------------------------------------------------------------------------------- 2: bit set, all rows equal
@pytest.mark.parametrize("name, dtype", ALL)
def test_equal_rows_with_the_bit_give_the_bits_of_the_shared_launch(name, dtype):
    fam = PB.family(name)
    k = 1                                                   # a row without a fixed parameter; the starts are clipped into it
    lo, up = fam.lo[k], fam.up[k]
    x0 = np.clip(fam.x0, lo, up)
    for variant in sorted({v for inst in ("default", "bounded") for v in variants_of(fam, inst)}):
        for w in (None, PB.weights_for(fam)):
            shared = PB.fit_family(fam, dtype, variant=variant, w=w, lo=lo, up=up, x0=x0, cov=True)
            tiled = PB.fit_family(fam, dtype, variant=variant, w=w, lo=np.tile(lo, (fam.count, 1)), up=np.tile(up, (fam.count, 1)),
                                  x0=x0, cov=True)
            assert fam.wide or variant == 0 or shared[0]["iterations"].sum() > fam.count
            assert same(shared, tiled)
            assert PB.bits(shared[2]).tobytes() == PB.bits(tiled[2]).tobytes()       # and the covariance kernels


# ------------------------------------------------------------------------------------------------------------ 3: the oracle
@pytest.mark.parametrize("name, dtype", ALL)
def test_fits_match_the_oracle_with_each_problems_own_box(oracle, name, dtype):
    """Problem k against oracle.optimize with row k, at the project's bars; every fixed parameter comes back with the bits of
    its bound, every x lies inside its own box. n <= 8: the bounded instance (the default one leaves -100).
    The 16-lane families as tests/test_gpu_batched16.py treats its bounded fits: the problems on which the oracle's own two
    summation orders (rows reversed) disagree beyond the tight bar are not counted against the 95 % -- on the CPU alone that is
    problems 2, 7 of PB16h (x apart by up to 9.4e-5 relative), 4 of PB16h9 (2.2e-5) and 0, 9, 10, 12 of PB16g (3.0e-4): flat
    constrained valleys, the residuals agree to 1.8e-9. Unlike there, those problems are still held to the outer bar here
    (status class, residual 1e-7, x 1e-3 / 1e-4), and every residual to the 1e-6 of that test. Measured on the MI355X against the
    first order: PB16h 0 of 16 outside the tight bar, PB16h9 problem 4 (2.2e-5), PB16g problems 10 and 12 (2.0e-5)."""
    fam = PB.family(name)
    ref = PB.oracle_fits(oracle, name, dtype)
    assert all(r.status >= 0 for r, _ in ref)
    aside = PB.self_disagreeing(ref, PB.oracle_fits(oracle, name, dtype, reverse=True)) if fam.wide else set()
    lo, up = fam.lo.astype(dtype), fam.up.astype(dtype)
    for variant in variants_of(fam, "bounded"):
        raw, x, _ = PB.fit_family(fam, dtype, variant=variant)
        label = f"{name} {np.dtype(dtype).name} variant {variant}"
        print(f"{label}: statuses {np.unique(raw['status'], return_counts=True)}")
        assert np.all(x >= lo) and np.all(x <= up)
        assert fam.fixed.any() and PB.bits(x[fam.fixed]).tobytes() == PB.bits(lo[fam.fixed]).tobytes()
        if dtype == F64:
            PB.compare_f64(label, raw, x, ref, aside)
            if fam.wide:
                assert all(abs(raw["residual"][k] / ref[k][0].residual - 1) <= 1e-6 for k in range(fam.count))
        else:
            PB.compare_f32(label, name, raw, x, ref)


# ------------------------------------------------------------------------------------------------ 4: per-problem validation
@pytest.mark.parametrize("name, dtype", ALL)
def test_a_start_outside_its_own_box_is_that_problems_bounds_error(name, dtype):
    """problem j starts at problem 0's start: inside box 0, outside its own -> -32 for j alone; nobody else changes a bit"""
    fam = PB.family(name)
    lo, up = fam.lo.astype(dtype), fam.up.astype(dtype)
    s0 = fam.x0[0].astype(dtype)
    assert np.all(s0 >= lo[0]) and np.all(s0 <= up[0])
    j = next(k for k in range(1, fam.count) if np.any(s0 < lo[k]) or np.any(s0 > up[k]))
    x0 = fam.x0.copy()
    x0[j] = fam.x0[0]
    variant = variants_of(fam, "bounded")[0]
    base = PB.fit_family(fam, dtype, variant=variant)
    moved = PB.fit_family(fam, dtype, variant=variant, x0=x0)
    assert moved[0]["status"][j] == -32, (j, moved[0]["status"])
    assert base[0]["status"][j] >= 0
    keep = np.arange(fam.count) != j
    assert moved[0][keep].tobytes() == base[0][keep].tobytes() and moved[1][keep].tobytes() == base[1][keep].tobytes()
    assert moved[1][j].tobytes() == x0[j].astype(dtype).tobytes()            # the refused problem's x is untouched


# ----------------------------------------------------------------------------------------------------------- 5: host entry
@pytest.mark.parametrize("name, dtype", SMALL)
def test_host_entry_completes_the_bounded_problems_with_their_own_rows(name, dtype):
    """without BATCHED_DEVICE_BOUNDS the general solver finishes the -100 problems, each in its own box: no -100 is left and the
    result agrees with the DEVICE_BOUNDS launch at the existing float / double bars"""
    fam = PB.family(name)
    kernel_default = PB.fit_family(fam, dtype)
    assert np.any(kernel_default[0]["status"] == -100)
    res, x = M.optimizeLeastSquaresBatched(fam.model, fam.x0, fam.t, fam.data, l=fam.lo, u=fam.up, dtype=dtype)
    status = np.array([int(r.status) for r in res])
    print(f"{name} {np.dtype(dtype).name}: {int((kernel_default[0]['status'] == -100).sum())} problems completed by the general solver")
    assert np.all(status >= 0), status
    lo, up = fam.lo.astype(dtype), fam.up.astype(dtype)
    assert np.all(x >= lo) and np.all(x <= up)
    assert PB.bits(x[fam.fixed]).tobytes() == PB.bits(lo[fam.fixed]).tobytes()
    raw, xb, _ = PB.fit_family(fam, dtype, variant=PB.DEVICE_BOUNDS)
    host = np.zeros(fam.count, dtype=PB.rdt(dtype))
    host["status"] = status; host["residual"] = [r.residual for r in res]
    ref = [(PB.Rec(raw[k]), xb[k]) for k in range(fam.count)]
    label = f"{name} {np.dtype(dtype).name}, host entry against the DEVICE_BOUNDS launch"
    if dtype == F64:
        PB.compare_f64(label, host, x, ref)
    else:
        PB.compare_f32(label, name, host, x, ref)
    # and with the bit the host entry returns the kernel entry's bits
    res_b, x_b = M.optimizeLeastSquaresBatched(fam.model, fam.x0, fam.t, fam.data, l=fam.lo, u=fam.up, dtype=dtype, variant=PB.DEVICE_BOUNDS)
    assert x_b.tobytes() == xb.tobytes() and [int(r.status) for r in res_b] == raw["status"].tolist()


def test_host_entries_of_the_16_lane_kernel_return_the_kernel_entrys_bits():
    for name in ("PB16h", "PB16g"):
        fam = PB.family(name)
        raw, x, cov = PB.fit_family(fam, F64, cov=True)
        res, xh = M.optimizeLeastSquaresBatched(fam.model, fam.x0, fam.t, fam.data, l=fam.lo, u=fam.up, dtype=F64)
        assert xh.tobytes() == x.tobytes() and [int(r.status) for r in res] == raw["status"].tolist()
        res, xh, ch = M.optimizeLeastSquaresBatched16(fam.model, fam.x0, fam.t, fam.data, l=fam.lo, u=fam.up, covariance=True)
        assert xh.tobytes() == x.tobytes() and PB.bits(ch).tobytes() == PB.bits(cov).tobytes()


# ------------------------------------------------------------------------------------------- 6: covariance, fixed parameters
@pytest.mark.parametrize("name, dtype", ALL)
def test_covariance_with_fixed_parameters_against_numpy_on_the_free_columns(name, dtype):
    fam = PB.family(name)
    fixed_problems = fam.fixed.any(axis=1)
    assert fixed_problems.any() and not fixed_problems.all()
    # the same boxes with every fixed parameter's box opened: problems without one must keep their bits
    lo_open, up_open = np.where(fam.fixed, -np.inf, fam.lo), np.where(fam.fixed, np.inf, fam.up)
    for variant in variants_of(fam, "bounded"):
        raw, x, cov, cov_alone = PB.fit_family(fam, dtype, variant=variant, cov=True, cov_only=True)
        assert np.all(raw["status"] >= 0)
        gap, cond = PB.covariance_gaps(fam, x, cov)
        bar = 100 * 2.0 ** -52 * cond if variant & PB.ANALYTIC and fam.wide else FD_BAR[(name, dtype)]
        print(f"covariance {name} {np.dtype(dtype).name} variant {variant}: worst scaled gap on the free block {gap:.3e} (bar {bar:.1e}; "
              f"cond {cond:.2e})")
        assert PB.bits(cov_alone).tobytes() == PB.bits(cov).tobytes()         # the covariance entry alone: the same bits
        for k in np.flatnonzero(fixed_problems):
            free = ~fam.fixed[k]
            assert np.all(np.diag(cov[k])[free] > 0), (k, cov[k])
        _, x_open, cov_open = PB.fit_family(fam, dtype, variant=variant, cov=True, lo=lo_open, up=up_open)
        keep = ~fixed_problems
        assert x_open[keep].tobytes() == x[keep].tobytes() and PB.bits(cov_open[keep]).tobytes() == PB.bits(cov[keep]).tobytes()
        assert gap <= bar, (gap, bar)


# ------------------------------------------------------------------------------------------------------ 7: degrees of freedom
@pytest.mark.parametrize("name, dtype", ALL)
def test_degrees_of_freedom_count_the_free_parameters(name, dtype):
    """zero weights leave exactly n rows: with one parameter fixed the free block is finite (rows - n_free = 1), with that
    parameter's box opened every entry is +inf -- with and without ABSOLUTE_SIGMA (the covariance entries on hand-made records:
    status 1, residual 1, x = the start)"""
    fam = PB.family(name)
    k = int(np.flatnonzero(fam.fixed.any(axis=1))[0])
    j = int(np.flatnonzero(fam.fixed[k])[0])
    rows = np.unique(np.round(np.linspace(2, fam.m - 3, fam.n)).astype(int))
    assert rows.size == fam.n
    w = np.zeros(fam.m); w[rows] = 1.0
    recs = np.zeros(1, dtype=PB.rdt(dtype)); recs["status"] = 1; recs["residual"] = 1.0
    fn, model = PB.covariance_entry(fam, dtype)
    lo_open, up_open = fam.lo[k].copy(), fam.up[k].copy()
    lo_open[j], up_open[j] = -np.inf, np.inf
    variant = PB.ANALYTIC if fam.has_grad else 0
    for flags in (0, PB.ABSOLUTE_SIGMA):
        for per_problem in (False, True):
            box = (lambda a: a[None, :]) if per_problem else (lambda a: a)
            args = dict(variant=variant, flags=flags, w=w, recs=recs, fit=False, per_problem=per_problem)
            _, _, cov = PB.launch(fn, model, dtype, fam.x0[k:k + 1], fam.t, fam.data[k:k + 1], box(fam.lo[k]), box(fam.up[k]), **args)
            free = ~fam.fixed[k]
            assert np.all(cov[0][~free, :] == 0) and np.all(cov[0][:, ~free] == 0), cov[0]
            block = cov[0][np.ix_(free, free)]
            assert np.all(np.isfinite(block)) and np.all(np.diag(block) > 0), (flags, cov[0])
            _, _, cov = PB.launch(fn, model, dtype, fam.x0[k:k + 1], fam.t, fam.data[k:k + 1], box(lo_open), box(up_open), **args)
            assert np.all(cov == np.inf), (flags, cov[0])


def test_infinite_entries_fill_the_free_block_only():
    """a free minor that is not positive: EXP_DECAY at p0 = 0 has a zero rate column; with p2 fixed the free entries are +inf
    and row / column 2 stay 0. A negative status is NaN everywhere, as always."""
    fam = PB.family("PB3")
    recs = np.zeros(2, dtype=PB.rdt(F64)); recs["status"] = [1, -26]; recs["residual"] = 1.0
    x = np.array([[0.0, 1.0, 0.2], [1.0, 1.0, 0.2]])
    lo = np.array([[-np.inf, -np.inf, 0.2]] * 2); up = np.array([[np.inf, np.inf, 0.2]] * 2)
    fn, model = PB.covariance_entry(fam, F64)
    _, _, cov = PB.launch(fn, model, F64, x, fam.t, fam.data[:2], lo, up, recs=recs, fit=False)
    assert np.all(cov[0][:2, :2] == np.inf) and np.all(cov[0][2, :] == 0) and np.all(cov[0][:, 2] == 0), cov[0]
    assert np.all(np.isnan(cov[1])), cov[1]


# ------------------------------------------------------------------------------------------------------ 8: the device header
def peak_problems(count=16, m=70):
    """the caller's model of tests/user_model/user_model_problem_bounds.hip, p0 exp(-((t - p1) / p2)^2 / 2) + p3, with the
    peak position in a window of +-0.3 around each spectrum's own maximum, the width >= .05, and on every fourth problem the
    baseline FIXED at a value .02 above the truth"""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 4))
    lo = np.full((count, 4), -np.inf); up = np.full((count, 4), np.inf)
    for k in range(count):
        u = P.splitmix64_uniform(5200 + k, m + 8)
        p = np.array([1.0 + u[0], 1.0 + 2.0 * u[1], 0.25 + 0.2 * u[2], 0.2 * u[3]])
        data[k] = p[0] * np.exp(-0.5 * ((t - p[1]) / p[2]) ** 2) + p[3] + 0.01 * (2 * u[8:] - 1)
        x0[k] = p * (1 + 0.1 * (2 * u[4:8] - 1))
        peak = t[np.argmax(data[k])]
        lo[k, 1], up[k, 1] = peak - 0.3, peak + 0.3
        lo[k, 2] = 0.05
        if k % 4 == 3:
            lo[k, 3] = up[k, 3] = p[3] + 0.02
    return t, data, np.clip(x0, lo, up), lo, up


@pytest.mark.parametrize("dtype", [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")])
def test_user_model_with_a_box_per_problem_matches_the_oracle(oracle, dtype):
    """launch_batched_bounded<Model> with the flag in its extras. double: the bar of tests/test_gpu_user_model_f64.py (`agree`);
    float: the bar of tests/test_gpu_user_model.py (residual 1e-3; |x - x_o| / max(1, |x_o|): median 1e-4, 99 % 5e-3, max 5e-2)"""
    t, data, x0, lo, up = peak_problems()
    fn = getattr(PB.user_lib_peaks(), "user_fit_peak_window_" + PB.suffix(dtype))
    raw, x, cov = PB.launch(fn, None, dtype, x0, t, data, lo, up, cov=True)
    assert np.all(raw["status"] >= 0), raw["status"]
    lo_t, up_t = lo.astype(dtype), up.astype(dtype)
    fixed = lo == up
    assert np.all(x >= lo_t) and np.all(x <= up_t) and PB.bits(x[fixed]).tobytes() == PB.bits(lo_t[fixed]).tobytes()
    assert np.all(cov[fixed.any(axis=1)][:, 3, :] == 0) and np.all(cov[fixed.any(axis=1)][:, :, 3] == 0) and np.all(np.isfinite(cov))
    tt = t.astype(dtype)
    ref = []
    for k in range(x0.shape[0]):
        d = data[k].astype(dtype)

        def f(p, y, d=d):
            y[:] = p[0] * np.exp(dtype(-0.5) * ((tt - p[1]) / p[2]) ** 2) + p[3] - d
        ref.append(oracle.optimize(f, t.size, x0[k].astype(dtype), lower=lo_t[k], upper=up_t[k], settings=oracle.default_settings(dtype),
                                   dtype=dtype))
    assert all(r.status >= 0 for r, _ in ref)
    if dtype == F64:
        PB.compare_f64("user model, a box per problem, f64", raw, x, ref)
        return
    xo = np.array([xk for _, xk in ref], dtype=F64)
    rerr = np.abs(raw["residual"].astype(F64) / np.array([r.residual for r, _ in ref]) - 1)
    errs = (np.abs(x.astype(F64) - xo) / np.maximum(1.0, np.abs(xo))).max(axis=1)
    print(f"user model, a box per problem, f32: residual gap max {rerr.max():.3e}; x err median {np.median(errs):.3e} "
          f"q99 {np.quantile(errs, 0.99):.3e} max {errs.max():.3e}")
    assert rerr.max() < 1e-3
    assert np.median(errs) < 1e-4 and np.quantile(errs, 0.99) < 5e-3 and errs.max() < 5e-2, (np.median(errs), errs.max())
