"""Problem families, launchers and references of the batched fits with PER-PROBLEM bounds and FIXED parameters
(MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM; tests/test_gpu_batched_problem_bounds.py, tests/test_batched_problem_bounds_host.py,
scripts/batched_problem_bounds.py; not a test module). Every family is seeded through problems.splitmix64_uniform, every box is
count x n (row k the box of problem k) and every start is clipped into its own box. With the oracle alone (CPU) every problem of
every family ends with status 0 or 1, in float and in double for the n <= 8 families and in double for the n = 16 ones.

  PB3    MODEL_EXP_DECAY, 24 problems, m = 70 (no multiple of the wave: one full and one partial row chunk), seeds 4100 + k:
         p = (1 + u0, .5 + 2 u1, .2 u2), noise .01 (2 u[6:] - 1), start p (1 + .1 (2 u[3:6] - 1)).
           k % 3 == 0   p1 in [p1* + .2, p1* + 1]: the window excludes the truth, the lower bound binds
           k % 3 == 1   p1 in [p1* - .5, p1* + .5]: nothing binds
           k % 3 == 2   p2 FIXED at p2* + .05 and p0 <= p0* - .1
         The oracle leaves 1 / 0 / 2 parameters on a bound, in that order of k % 3.
  PB8    MODEL_EXP_DECAY_PAD8, 24 problems, m = 70: make_pad8(24, 70, 900) of tests/test_gpu_batched_bounds.py restated, in that
         file's box B8_LOWER / B8_UPPER with p1 in [1 + .02 k, 2 - .02 k], p3 .. p6 in +-(.05 + .005 k) and p7 FIXED at 0 for
         k % 4 == 3. Between 1 and 5 parameters of every problem end on a bound.
  PB16h  MODEL16_EXP_HARM16 (n = 16) and the caller's Harm<9> (n = 9): harm_problems(n, 67, 16) of tests/batched16_problems.py;
         p_j in +-(.1 + .01 k) for j >= 3, p1 in [p1* + .1, p1* + 1] for k % 3 == 0, p2 FIXED at p2* + .02 for k % 4 == 3.
  PB16g  MODEL16_GAUSS3_AFFINE (n = 11): gauss3_problems(130, 16); centres in c_g +- (.15 + .005 k) with c = (.9, 2.1, 3.2),
         widths >= .05, p0 <= .8 x0_0 for k % 3 == 0, p10 FIXED at 0 for k % 4 == 3.

The parity bars are the project's, restated: `agree` / `compare_f64` / `compare_f32` of tests/test_gpu_batched_bounds.py and
`compare` of tests/test_gpu_batched16.py."""
import ctypes as C
import functools

import numpy as np

import mir_optim_amd as M
from mir_optim_amd import api, build as hipbuild
import problems as P
import weighted_problems as WP
import batched16_weighted_problems as WP16
from batched16_problems import gauss3_problems, gauss3_value, harm_basis, harm_problems, harm_value

PER_PROBLEM = 2            # MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM
ABSOLUTE_SIGMA = 1         # MIR_LSQ_BATCHED_ABSOLUTE_SIGMA
ANALYTIC = 2               # MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN
DEVICE_BOUNDS = 4          # MIR_LSQ_BATCHED_DEVICE_BOUNDS
B8_LOWER = np.array([-np.inf, 1.0, 0.0, -0.1, -0.1, -0.1, -0.1, -np.inf])
B8_UPPER = np.array([np.inf, 2.0, np.inf, 0.1, 0.1, 0.1, 0.1, np.inf])
M8 = 70


def rdt(dtype):
    f = "<f4" if dtype == np.float32 else "<f8"
    return np.dtype([("status", "<i4"), ("iterations", "<u4"), ("fCalls", "<u4"), ("gCalls", "<u4"), ("residual", f), ("lambda", f)])


def suffix(dtype):
    return "s" if dtype == np.float32 else "d"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------------------------ families
class Family:
    """model: the MIR_LSQ_MODEL* id, or None for a caller's model (entry: the name of its library's entry). All arrays float64,
    shared by the tests and never written. value(p) and jacobian(p) evaluate on the family's t."""
    def __init__(self, name, model, t, data, x0, lo, up, value, jacobian, has_grad=False, entry=None):
        self.name, self.model, self.entry, self.has_grad = name, model, entry, has_grad
        self.t, self.data, self.lo, self.up = t, data, lo, up
        self.x0 = np.clip(x0, lo, up)
        self.value, self.jacobian = value, jacobian
        self.count, self.n = self.x0.shape
        self.m = t.size
        self.wide = self.n > 8
        for a in (self.t, self.data, self.x0, self.lo, self.up):
            a.setflags(write=False)

    @property
    def fixed(self):
        return self.lo == self.up


def make_pad8(count, m, seed0, noise=0.01):
    """make_pad8 of tests/test_gpu_batched_bounds.py"""
    t = np.linspace(0.0, 4.0, m)
    data = np.empty((count, m)); x0 = np.empty((count, 8))
    basis = np.stack([np.sin(2 * t), np.cos(2 * t), np.sin(5 * t), np.cos(5 * t), t])
    for k in range(count):
        u = P.splitmix64_uniform(seed0 + k, m + 16)
        p = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2], 0.6 * u[3] - 0.3, 0.6 * u[4] - 0.3, 0.6 * u[5] - 0.3,
                      0.6 * u[6] - 0.3, 0.1 * u[7] - 0.05])
        data[k] = p[0] * np.exp(-t * p[1]) + p[2] + p[3:] @ basis + noise * (2 * u[16:] - 1)
        x0[k] = p
        x0[k, :2] *= 1 + 0.2 * (2 * u[8:10] - 1)
        x0[k, 2:] += 0.1 * (2 * u[10:16] - 1)
    return t, data, x0


def _harm_boxes(n, truth):
    count = truth.shape[0]
    lo = np.full((count, n), -np.inf); up = np.full((count, n), np.inf)
    for k in range(count):
        lo[k, 3:] = -(0.1 + 0.01 * k); up[k, 3:] = 0.1 + 0.01 * k
        if k % 3 == 0:
            lo[k, 1] = truth[k, 1] + 0.1; up[k, 1] = truth[k, 1] + 1.0
        if k % 4 == 3:
            lo[k, 2] = up[k, 2] = truth[k, 2] + 0.02
    return lo, up


@functools.lru_cache(maxsize=None)
def family(name):
    if name == "PB3":
        count, m = 24, M8
        t = np.linspace(0.0, 4.0, m)
        data = np.empty((count, m)); x0 = np.empty((count, 3))
        lo = np.full((count, 3), -np.inf); up = np.full((count, 3), np.inf)
        for k in range(count):
            u = P.splitmix64_uniform(4100 + k, m + 6)
            p = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2]])
            data[k] = p[0] * np.exp(-t * p[1]) + p[2] + 0.01 * (2 * u[6:] - 1)
            x0[k] = p * (1 + 0.1 * (2 * u[3:6] - 1))
            if k % 3 == 0:
                lo[k, 1] = p[1] + 0.2; up[k, 1] = p[1] + 1.0
            elif k % 3 == 1:
                lo[k, 1] = p[1] - 0.5; up[k, 1] = p[1] + 0.5
            else:
                lo[k, 2] = up[k, 2] = p[2] + 0.05
                up[k, 0] = p[0] - 0.1
        return Family(name, M.MODEL_EXP_DECAY, t, data, x0, lo, up, lambda p: WP.model_value(WP.EXP_DECAY, t, p),
                      lambda p: WP.model_jacobian(WP.EXP_DECAY, t, p))
    if name == "PB8":
        count = 24
        t, data, x0 = make_pad8(count, M8, 900)
        lo = np.tile(B8_LOWER, (count, 1)); up = np.tile(B8_UPPER, (count, 1))
        for k in range(count):
            lo[k, 1] = 1 + 0.02 * k; up[k, 1] = 2 - 0.02 * k
            lo[k, 3:7] = -(0.05 + 0.005 * k); up[k, 3:7] = 0.05 + 0.005 * k
            if k % 4 == 3:
                lo[k, 7] = up[k, 7] = 0.0
        return Family(name, M.MODEL_EXP_DECAY_PAD8, t, data, x0, lo, up, lambda p: WP.model_value(WP.PAD8, t, p),
                      lambda p: WP.model_jacobian(WP.PAD8, t, p))
    if name in ("PB16h", "PB16h9"):
        n = 16 if name == "PB16h" else 9
        t, B, data, truth, x0 = harm_problems(n, 67, 16)
        lo, up = _harm_boxes(n, truth)
        return Family(name, M.MODEL16_EXP_HARM16 if n == 16 else None, t, data, x0, lo, up, lambda p: harm_value(B, t, p),
                      lambda p: WP16.harm_jacobian(B, t, p), has_grad=True, entry="user_fit_weighted_harm9_d")
    if name == "PB16g":
        count = 16
        t, data, x0 = gauss3_problems(130, count)
        lo = np.full((count, 11), -np.inf); up = np.full((count, 11), np.inf)
        for k in range(count):
            for g, c in enumerate((0.9, 2.1, 3.2)):
                lo[k, 3 * g + 1] = c - (0.15 + 0.005 * k); up[k, 3 * g + 1] = c + (0.15 + 0.005 * k)
                lo[k, 3 * g + 2] = 0.05
            if k % 3 == 0:
                up[k, 0] = 0.8 * x0[k, 0]
            if k % 4 == 3:
                lo[k, 10] = up[k, 10] = 0.0
        return Family(name, M.MODEL16_GAUSS3_AFFINE, t, data, x0, lo, up, lambda p: gauss3_value(t, p),
                      lambda p: WP16.gauss3_jacobian(t, p))
    raise KeyError(name)


def weights_for(fam, zero_tail=True):
    """per-row weights shared by the problems of a family: .5 + u, the last 7 rows at weight 0 (zero_tail)"""
    w = 0.5 + P.splitmix64_uniform(77, fam.m)
    if zero_tail:
        w[-7:] = 0.0
    return w


# ------------------------------------------------------------------------------------------------------------------- launches
@functools.lru_cache(maxsize=None)
def user_lib16():
    UL = C.CDLL(hipbuild.user_model_n16_weighted_lib())
    for name in ("user_fit_weighted_harm9_d", "user_weighted_harm9_covariance_d"):
        fn = getattr(UL, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 4
    return UL


@functools.lru_cache(maxsize=None)
def user_lib_peaks():
    UL = C.CDLL(hipbuild.user_model_problem_bounds_lib())
    for name in ("user_fit_peak_window_s", "user_fit_peak_window_d"):
        fn = getattr(UL, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 4
    return UL


def fit_entry(fam, dtype, plain16=False):
    """(function, model argument or None) of the device-pointer fit entry of a family. plain16: the batched16 entry without
    _ex (it takes an extras that carries flags only)"""
    if fam.model is None:
        return getattr(user_lib16(), fam.entry), None
    if fam.wide:
        return (api.lib().mir_lsq_batched16_kernel_d if plain16 else api.lib().mir_lsq_batched16_kernel_ex_d), int(fam.model)
    return getattr(api.lib(), "mir_lsq_batched_kernel_ex_" + suffix(dtype)), int(fam.model)


def covariance_entry(fam, dtype):
    if fam.model is None:
        return user_lib16().user_weighted_harm9_covariance_d, None
    if fam.wide:
        return api.lib().mir_lsq_batched16_covariance_d, int(fam.model)
    return getattr(api.lib(), "mir_lsq_batched_covariance_" + suffix(dtype)), int(fam.model)


def launch(fn, model, dtype, x0, t, data, lo, up, variant=0, flags=0, w=None, cov=False, per_problem=None, cov_fn=None, recs=None,
           fit=True):
    """One launch of a device-pointer entry that takes extras, on device data; the basis table is the call's own. lo / up: n
    values or count x n; per_problem (default: lo is 2-D) sets MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM. Returns (records, x, cov or
    None) -- and, with cov_fn (a covariance-only entry of the same signature), that entry's result on the device data the
    launch left as a fourth value. fit=False: fn is a covariance-only entry itself, run on x0 and the records `recs`."""
    count, n = x0.shape
    m = data.shape[1]
    x0, t, data, lo, up = (np.ascontiguousarray(a, dtype=dtype) for a in (x0, t, data, lo, up))
    if per_problem is None:
        per_problem = lo.ndim == 2
    assert lo.shape == up.shape == ((count, n) if per_problem else (n,)), (lo.shape, up.shape)
    s = M.LeastSquaresSettings(dtype)
    R = rdt(dtype)
    t_stride = 0 if t.ndim == 1 else m
    bufs = [api.DeviceBuffer(a) for a in (t, data, x0, lo, up)]
    dt_, dd, dx, dlo, dup = bufs
    pattern = np.full(count * R.itemsize, 0x5A, np.uint8) if recs is None else np.ascontiguousarray(recs).view(np.uint8)
    dres = api.DeviceBuffer(pattern)
    bufs.append(dres)
    dcov = dw = None
    if cov or cov_fn is not None or not fit:
        dcov = api.DeviceBuffer(np.full((count, n, n), 7.0, dtype))
        bufs.append(dcov)
    if w is not None:
        w = np.ascontiguousarray(w, dtype=dtype)
        dw = api.DeviceBuffer(w)
        bufs.append(dw)
    st = api.Stream()
    opt = api.BatchedOptions(stream=st.handle, variant=variant)
    ex = api.BatchedExtras(flags=flags | (PER_PROBLEM if per_problem else 0), weights=dw.ptr if dw else None,
                           weight_stride=0 if (w is None or w.ndim == 1) else m, covariance=dcov.ptr if (cov or not fit) else None)
    head = [C.byref(s), count, m] + ([model] if model is not None else [])
    rc = fn(*head, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr, dres.ptr, C.byref(opt), C.byref(ex))
    assert rc == 0, rc
    st.synchronize()
    out = [np.frombuffer(dres.download().tobytes(), dtype=R).copy(), dx.download().reshape(count, n).copy(),
           dcov.download().reshape(count, n, n).copy() if (cov or not fit) else None]
    if cov_fn is not None:
        dcov.upload(np.full((count, n, n), 7.0, dtype))
        ex.covariance = dcov.ptr
        rc = cov_fn(*head, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, t_stride, dd.ptr, dres.ptr, C.byref(opt), C.byref(ex))
        assert rc == 0, rc
        st.synchronize()
        out.append(dcov.download().reshape(count, n, n).copy())
    for b in bufs:
        b.free()
    return tuple(out)


def fit_family(fam, dtype, variant=0, flags=0, w=None, cov=False, own_t=False, lo=None, up=None, x0=None, plain16=False,
               cov_only=False, per_problem=None):
    fn, model = fit_entry(fam, dtype, plain16)
    t = np.tile(fam.t, (fam.count, 1)) if own_t else fam.t
    return launch(fn, model, dtype, fam.x0 if x0 is None else x0, t, fam.data, fam.lo if lo is None else lo,
                  fam.up if up is None else up, variant=variant, flags=flags, w=w, cov=cov, per_problem=per_problem,
                  cov_fn=covariance_entry(fam, dtype)[0] if cov_only else None)


def fit_one(fam, k, dtype, variant=0, w=None, own_t=False, plain16=False):
    """problem k alone (count = 1) with row k as the SHARED box of the launch"""
    fn, model = fit_entry(fam, dtype, plain16)
    t = fam.t[None, :] if own_t else fam.t
    return launch(fn, model, dtype, fam.x0[k:k + 1], t, fam.data[k:k + 1], fam.lo[k], fam.up[k], variant=variant, w=w)


# ------------------------------------------------------------------------------------------------------------------ references
_ORACLE = {}


def oracle_fits(oracle, name, dtype, reverse=False):
    """the oracle's fit of every problem of a family with ITS OWN row as the box, in `dtype` (a Python f evaluating the model in
    that precision), computed once a session: [(result, x)]. reverse: the rows in the opposite order (another summation order)"""
    key = (name, np.dtype(dtype).name, reverse)
    if key not in _ORACLE:
        fam = family(name)
        tt = (fam.t[::-1].copy() if reverse else fam.t).astype(dtype)
        if fam.wide:
            B = harm_basis(fam.n, tt) if name.startswith("PB16h") else None
            value = (lambda p: harm_value(B, tt, p)) if B is not None else (lambda p: gauss3_value(tt, p))
        else:
            value = lambda p: WP.model_value(fam.model, tt, p)                  # noqa: E731
        out = []
        for k in range(fam.count):
            d = (fam.data[k][::-1].copy() if reverse else fam.data[k]).astype(dtype)

            def f(p, y, d=d):
                y[:] = value(p) - d
            out.append(oracle.optimize(f, fam.m, fam.x0[k].astype(dtype), lower=fam.lo[k].astype(dtype), upper=fam.up[k].astype(dtype),
                                       settings=oracle.default_settings(dtype), dtype=dtype))
        _ORACLE[key] = out
    return _ORACLE[key]


class Rec:
    def __init__(self, row):
        self.status, self.residual = int(row["status"]), float(row["residual"])


def agree(k, status, residual, x, rr, xr, loose):
    """`agree` of tests/test_gpu_batched_bounds.py for one problem against the reference rr, xr"""
    assert (status >= 0) == (rr.status >= 0), (k, status, rr.status)
    if rr.status < 0:
        return 0.0, 0.0
    tight = np.allclose(x, xr, rtol=1e-6, atol=1e-7)
    near = np.allclose(x, xr, rtol=1e-3, atol=1e-4)
    gap = float(np.max(np.abs(x - xr) / np.maximum(np.abs(xr), 1e-3)))
    rgap = abs(residual / rr.residual - 1)
    if not (tight and rgap <= 1e-9):
        loose.append((k, gap, rgap))
        assert near and rgap <= 1e-7, (k, gap, rgap, x, xr)
    return gap, rgap


def compare_f64(label, raw, x, ref, aside=()):
    """the f64 bar of tests/test_gpu_batched_bounds.py (and, on the same numbers, `compare` of tests/test_gpu_batched16.py): the
    same status class on every problem, residual to 1e-9 and x to 1e-6 / 1e-7 on at least 95 % of the problems, the rest within
    1e-7 / 1e-3 (1e-4). ref = [(result, x)] per problem. aside: problems that are not counted against the 95 % (they are still
    held to the status class and to 1e-7 / 1e-3: see self_disagreeing)"""
    loose = []
    assert np.all(raw["status"] != -100), raw["status"]
    gaps = [agree(k, int(raw["status"][k]), float(raw["residual"][k]), x[k], rr, xr, loose) for k, (rr, xr) in enumerate(ref)]
    print(f"{label}: worst x gap {max(g for g, _ in gaps):.3e}, worst residual gap {max(r for _, r in gaps):.3e}, "
          f"{len(loose)} of {len(ref)} outside the tight bar: {loose}; set aside {sorted(aside)}")
    counted = [l for l in loose if l[0] not in aside]
    assert len(counted) <= 0.05 * (len(ref) - len(aside)), counted


def self_disagreeing(ref, again):
    """the problems on which the ORACLE, run twice with its rows in opposite orders, is outside the tight bar against itself
    (tests/test_gpu_batched16.py sets those aside for its bounded fits: test_bounded_fits_finish_in_the_kernel_and_match_the_
    bounded_oracle): no fit can be asked to agree with a reference more closely than the reference agrees with itself"""
    aside = set()
    for k, ((rr, xr), (r2, x2)) in enumerate(zip(ref, again)):
        if rr.status < 0 or r2.status < 0:
            continue
        if not (np.allclose(x2, xr, rtol=1e-6, atol=1e-7) and abs(r2.residual / rr.residual - 1) <= 1e-9):
            aside.add(k)
    return aside


def compare_f32(label, name, raw, x, ref):
    """the float bars of tests/test_gpu_batched_bounds.py: EXP_DECAY x rtol 5e-3, atol 5e-4 and residual rtol 5e-3; PAD8 residual
    rtol 1e-3 and |x - x_oracle| <= 5e-2 max(1, |x|)"""
    st_o = np.array([int(r.status) for r, _ in ref]); res_o = np.array([float(r.residual) for r, _ in ref])
    xo = np.array([xk for _, xk in ref], dtype=np.float64)
    assert np.array_equal(raw["status"] >= 0, st_o >= 0), (raw["status"], st_o)
    ok = st_o >= 0
    x = x.astype(np.float64); resid = raw["residual"].astype(np.float64)
    rgap = np.abs(resid[ok] / res_o[ok] - 1)
    err = (np.abs(x - xo) / np.maximum(1.0, np.abs(xo))).max(axis=1)[ok]
    print(f"{label}: residual gap max {rgap.max():.3e}; |x - x_oracle| / max(1, |x|) max {err.max():.3e}, "
          f"|x - x_oracle| max {np.abs(x - xo)[ok].max():.3e}")
    if name == "PB3":
        assert np.allclose(x[ok], xo[ok], rtol=5e-3, atol=5e-4) and np.allclose(resid[ok], res_o[ok], rtol=5e-3, atol=0)
    else:
        assert np.allclose(resid[ok], res_o[ok], rtol=1e-3, atol=0) and err.max() <= 5e-2


def reference_covariance(fam, k, x, w=None, absolute_sigma=False, fixed=None):
    """numpy float64: the covariance of the FREE parameters of problem k at x from the analytic Jacobian,
    inv(J_free^T J_free) ||w f(x)||^2 / (rows with a nonzero weight - n_free), embedded in n x n with zeros in the rows and
    columns of the fixed ones. Returns (cov, free mask, equilibrated condition number of the free J^T J)"""
    fixed = fam.fixed[k] if fixed is None else fixed
    free = ~fixed
    w = np.ones(fam.m) if w is None else np.asarray(w, dtype=np.float64)
    xk = np.asarray(x, dtype=np.float64)
    r = w * (fam.value(xk) - fam.data[k])
    J = (fam.jacobian(xk) * w[:, None])[:, free]
    A = J.T @ J
    inv = np.linalg.inv(A)
    d = 1.0 / np.sqrt(np.diag(A))
    cond = float(np.linalg.cond(A * np.outer(d, d)))
    s2 = 1.0 if absolute_sigma else float(r @ r) / (int(np.count_nonzero(w)) - int(free.sum()))
    cov = np.zeros((fam.n, fam.n))
    cov[np.ix_(free, free)] = s2 * inv
    return cov, free, cond


def covariance_gaps(fam, x, cov, w=None, absolute_sigma=False, fixed=None):
    """(worst gap of the free block scaled by sd_i sd_j, largest condition number); asserts, per problem: the rows and columns of
    the fixed parameters are exactly 0, the free block is finite, the matrix is symmetric to the bit"""
    worst = cond = 0.0
    for k in range(fam.count):
        ref, free, c = reference_covariance(fam, k, x[k], w, absolute_sigma, None if fixed is None else fixed[k])
        ck = np.asarray(cov[k], dtype=np.float64)
        assert np.all(cov[k][~free, :] == 0) and np.all(cov[k][:, ~free] == 0), (k, cov[k])
        assert np.all(np.isfinite(ck)), (k, cov[k])
        assert (bits(cov[k]) == bits(cov[k].T.copy())).all(), k
        sd = np.sqrt(np.diag(ref)[free])
        worst = max(worst, float(np.max(np.abs(ck - ref)[np.ix_(free, free)] / np.outer(sd, sd))))
        cond = max(cond, c)
    return worst, cond
