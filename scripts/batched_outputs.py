#!/usr/bin/env python3
"""Every output of every batched entry on a fixed set of small problems, in one file: the tool for comparing the HOST layer of
two trees whose kernels are the same (profiles/r20/host_layer_refactor.txt).

    python scripts/batched_outputs.py OUT.npz          (needs a GPU; run it in each tree, then compare the two files)

Calls, in the tree it lies in, the library's batched entries -- the device-pointer fit entries with and without extras, the
covariance entries and the host-pointer entries, _s and _d for the models of up to 8 parameters and _d for those of 9 to 16 --
and every user_* fit and covariance entry of the libraries of tests/user_model/ as they are built (nothing is compiled here),
and writes x, the result records (as bytes) and the covariance of every call into OUT.npz. The archive carries no time stamps:
two trees that compute the same give byte-equal files, and the SHA-256 that is printed says so at a glance.

Problems: the families of tests/batched16_problems.py, tests/weighted_problems.py and tests/problem_bounds_cases.py at
m = 33, 67, 131 (one, two and three 64-row passes; no multiples of 4) and count = 4 .. 8; n = 3, 8 (float and double), 9 (a
caller's model), 11 and 16; one box for the batch and a box per problem, with one parameter of problem 0 pushed onto its
bound; weights on and off, shared and per problem; covariance on and off; the analytic Jacobian where the model has grad; the
bounded kernels (MIR_LSQ_BATCHED_DEVICE_BOUNDS) and, without them, the host entry's completion of the bounded problems by the
general solver with the covariance behind it (also on the first problems of the family PB3 of problem_bounds_cases.py)."""
import ctypes as C
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mir_optim_amd as M  # noqa: E402
from mir_optim_amd import api  # noqa: E402
import batched16_problems as P16  # noqa: E402
import problem_bounds_cases as PB  # noqa: E402
import problems as P  # noqa: E402
import weighted_problems as WP  # noqa: E402

NO_ARGUMENT = object()          # the entry has no extras parameter
ROWS = (33, 67, 131)
OUT = {}


def record(name, recs, x, cov=None):
    assert name not in OUT, name
    OUT[name] = None
    OUT[name + "/records"] = np.frombuffer(np.ascontiguousarray(recs).tobytes(), np.uint8)
    OUT[name + "/x"] = np.ascontiguousarray(x)
    if cov is not None:
        OUT[name + "/cov"] = np.ascontiguousarray(cov)
    del OUT[name]


def device_call(fn, model, dtype, x, t, data, lo, up, variant=0, extras=None, recs=None):
    """One call of a device-pointer entry. extras: NO_ARGUMENT, None (a null pointer) or dict(flags, w, cov). recs: the records
    of an earlier fit (fn is then a covariance entry, which reads them and x). Returns (records, x, cov or None)."""
    count, n = x.shape
    m = data.shape[1]
    x, t, data, lo, up = (np.ascontiguousarray(a, dtype=dtype) for a in (x, t, data, lo, up))
    R = PB.rdt(dtype)
    bufs = [api.DeviceBuffer(a) for a in (t, data, x, lo, up)]
    dt_, dd, dx, dlo, dup = bufs
    dres = api.DeviceBuffer(np.full(count * R.itemsize, 0x5A, np.uint8) if recs is None else np.ascontiguousarray(recs).view(np.uint8))
    bufs.append(dres)
    tail = []
    dcov = None
    if extras is None:
        tail = [None]
    elif extras is not NO_ARGUMENT:
        ex = api.BatchedExtras(flags=extras.get("flags", 0) | (PB.PER_PROBLEM if lo.ndim == 2 else 0))
        w = extras.get("w")
        if w is not None:
            w = np.ascontiguousarray(w, dtype=dtype)
            bufs.append(api.DeviceBuffer(w))
            ex.weights = bufs[-1].ptr
            ex.weight_stride = 0 if w.ndim == 1 else m
        if extras.get("cov"):
            dcov = api.DeviceBuffer(np.full((count, n, n), 7.0, dtype))
            bufs.append(dcov)
            ex.covariance = dcov.ptr
        tail = [C.byref(ex)]
    st = api.Stream()
    s = M.LeastSquaresSettings(dtype)
    head = [C.byref(s), count, m] + ([int(model)] if model is not None else [])
    rc = fn(*head, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, 0 if t.ndim == 1 else m, dd.ptr, dres.ptr,
            C.byref(api.BatchedOptions(stream=st.handle, variant=variant)), *tail)
    assert rc == 0, rc
    st.synchronize()
    out = (np.frombuffer(dres.download().tobytes(), dtype=R).copy(), dx.download().reshape(count, n).copy(),
           dcov.download().reshape(count, n, n).copy() if dcov else None)
    for b in bufs:
        b.free()
    return out


def boxes(x0, per_problem):
    """(lo, up, x0 clipped): a box around every start with parameter 1 of problem 0 pushed onto its lower bound, or the one
    box that holds them all"""
    lo = x0 - 0.5 * np.abs(x0) - 0.05
    up = x0 + 0.5 * np.abs(x0) + 0.05
    lo[0, 1] = x0[0, 1] + 0.2 * abs(x0[0, 1])
    up[0, 1] = x0[0, 1] + abs(x0[0, 1]) + 0.3
    if not per_problem:
        lo = lo.min(axis=0); up = up.max(axis=0)
        lo[1] = x0[:, 1].max() * 1.05
        up[1] = lo[1] + 1.0
    return lo, up, np.clip(x0, lo, up)


def weights(count, m, per_problem):
    w = 0.5 + P.splitmix64_uniform(77, count * m).reshape(count, m)
    w[:, -3:] = 0.0
    return w if per_problem else w[0].copy()


def family(n, count, m):
    """(t, data, x0) of the family with n parameters"""
    if n == 3:
        return WP.exp_decay_weighted(count, m)[:3]
    if n == 8:
        return WP.pad8_weighted(count, m)[:3]
    if n == 11:
        return P16.gauss3_problems(m, count)
    t, _, data, _, x0 = P16.harm_problems(n, m, count)
    return t, data, np.array(x0)


def user_lib(name):
    return C.CDLL(os.path.join(ROOT, "tests", "user_model", "lib" + name + ".so"))


def user_fn(lib, name, extras):
    """an entry of an example: settings, count, m, x, lower, upper, t, t_stride, data, results, options[, extras]"""
    fn = getattr(lib, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * (4 if extras else 3)
    return fn


def library_entries(n, dtype, model, has_grad, count, m, tag):
    """every entry of the library for one built-in model on one problem set"""
    L = api.lib()
    wide = n > 8
    suf = PB.suffix(dtype)
    kernel = L.mir_lsq_batched16_kernel_d if wide else getattr(L, "mir_lsq_batched_kernel_" + suf)
    kernel_ex = L.mir_lsq_batched16_kernel_ex_d if wide else getattr(L, "mir_lsq_batched_kernel_ex_" + suf)
    cov_entry = L.mir_lsq_batched16_covariance_d if wide else getattr(L, "mir_lsq_batched_covariance_" + suf)
    t, data, x0 = family(n, count, m)
    t2 = np.tile(t, (count, 1)) * (1 + 1e-3 * np.arange(count))[:, None]           # a time axis per problem
    for per_problem in (False, True):
        lo, up, xs = boxes(np.array(x0, dtype=np.float64), per_problem)
        b = "own-box" if per_problem else "one-box"
        variants = [0] + ([] if wide else [PB.DEVICE_BOUNDS]) + ([PB.ANALYTIC] if has_grad else [])
        for variant in variants:
            v = "%s/%s/v%d" % (tag, b, variant)
            # the device-pointer entry without extras (a box per problem needs them: the wide one takes its flag, the other has no argument)
            if wide:
                record(v + "/kernel", *device_call(kernel, model, dtype, xs, t, data, lo, up, variant, {} if per_problem else None)[:2])
            elif not per_problem:
                record(v + "/kernel", *device_call(kernel, model, dtype, xs, t, data, lo, up, variant, NO_ARGUMENT)[:2])
            for wmode in (None, "shared", "own"):
                w = None if wmode is None else weights(count, m, wmode == "own")
                for cov in (False, True):
                    name = "%s/kernel_ex/w-%s/cov%d" % (v, wmode, cov)
                    tt = t2 if (wmode == "own" and cov) else t
                    recs, x, cv = device_call(kernel_ex, model, dtype, xs, tt, data, lo, up, variant,
                                              dict(w=w, cov=cov, flags=PB.ABSOLUTE_SIGMA if wmode == "shared" else 0))
                    record(name, recs, x, cv)
                    if cov:     # ... and the covariance entry on what that fit left
                        record(name + "/covariance_entry", *device_call(cov_entry, model, dtype, x, tt, data, lo, up, variant,
                                                                        dict(w=w, cov=True), recs=recs))
                    # the host-pointer entries, through the package: without DEVICE_BOUNDS the n <= 8 one completes bounded problems itself
                    fit = M.optimizeLeastSquaresBatched16 if wide else M.optimizeLeastSquaresBatched
                    kw = {} if wide else dict(dtype=dtype)
                    out = fit(model, xs, tt, data, l=lo, u=up, variant=variant, weights=w, covariance=cov,
                              absolute_sigma=wmode == "shared", **kw)
                    recs = np.array([(r.status, r.iterations, r.fCalls, r.gCalls, r.residual, r.lambda_) for r in out[0]], dtype=PB.rdt(dtype))
                    record(name.replace("kernel_ex", "host"), recs, out[1], out[2] if cov else None)


def completion_by_the_general_solver():
    """the first six problems of PB3 and PB8 (bounds that bind, fixed parameters) through the host entries without DEVICE_BOUNDS"""
    for fam_name in ("PB3", "PB8"):
        fam = PB.family(fam_name)
        k = 6
        for dtype in (np.float32, np.float64):
            for w in (None, PB.weights_for(fam)):
                out = M.optimizeLeastSquaresBatched(fam.model, fam.x0[:k], fam.t, fam.data[:k], l=fam.lo[:k], u=fam.up[:k], dtype=dtype,
                                                    weights=w, covariance=True)
                recs = np.array([(r.status, r.iterations, r.fCalls, r.gCalls, r.residual, r.lambda_) for r in out[0]], dtype=PB.rdt(dtype))
                record("%s/%s/host-completion/w%d" % (fam_name, PB.suffix(dtype), w is not None), recs, out[1], out[2])
                print("%s %s: statuses %s" % (fam_name, PB.suffix(dtype), [int(r.status) for r in out[0]]), flush=True)


def user_entries():
    """the examples of tests/user_model/: every user_* entry that launches a batched fit or its covariance"""
    plain = [("user_model", "user_fit_damped_cosine", np.float32, 6), ("user_model_f64", "user_fit_damped_cosine_d", np.float64, 5),
             ("user_model_bounded", "user_fit_logistic_bounded_d", np.float64, 4), ("user_model_bounded", "user_fit_logistic_bounded_s", np.float32, 4),
             ("user_model_bounded", "user_fit_logistic_d", np.float64, 4), ("user_model_n16", "user_fit_harm9_d", np.float64, 9),
             ("user_model_n16", "user_fit_harm13_d", np.float64, 13)]
    with_extras = [("user_model_weighted", "user_fit_weighted_peak_d", "user_weighted_peak_covariance_d", np.float64, 5),
                   ("user_model_weighted", "user_fit_weighted_peak_s", "user_weighted_peak_covariance_s", np.float32, 5),
                   ("user_model_problem_bounds", "user_fit_peak_window_d", None, np.float64, 4),
                   ("user_model_problem_bounds", "user_fit_peak_window_s", None, np.float32, 4),
                   ("user_model_n16_weighted", "user_fit_weighted_harm9_d", "user_weighted_harm9_covariance_d", np.float64, 9),
                   ("user_model_n16_weighted", "user_fit_weighted_harm13_d", "user_weighted_harm13_covariance_d", np.float64, 13)]
    for i, m in enumerate(ROWS):
        count = 4 + i
        for lib, name, dtype, n in plain:
            t, data, x0 = user_problem(n, count, m)
            lo, up, xs = boxes(x0, False)
            for variant in (0, PB.DEVICE_BOUNDS) if name == "user_fit_logistic_bounded_d" else (0,):
                record("%s/m%d/v%d" % (name, m, variant), *device_call(user_fn(user_lib(lib), name, False), None, dtype, xs, t, data, lo, up,
                                                                      variant, NO_ARGUMENT)[:2])
        for lib, name, cov_name, dtype, n in with_extras:
            t, data, x0 = user_problem(n, count, m)
            for per_problem in (False, True):
                lo, up, xs = boxes(x0, per_problem)
                for w in (None, weights(count, m, True)):
                    tag = "%s/m%d/box%d/w%d" % (name, m, per_problem, w is not None)
                    recs, x, cv = device_call(user_fn(user_lib(lib), name, True), None, dtype, xs, t, data, lo, up, 0, dict(w=w, cov=True))
                    record(tag, recs, x, cv)
                    if cov_name:
                        record(tag + "/covariance_entry", *device_call(user_fn(user_lib(lib), cov_name, True), None, dtype, x, t, data, lo, up, 0,
                                                                       dict(w=w, cov=True, flags=PB.ABSOLUTE_SIGMA), recs=recs))


def user_problem(n, count, m):
    """data for a caller's model of n parameters: the harmonic family where it is one (n = 9, 13), else a peak on a decaying
    baseline with noise, and starts near 1 -- the entries are compared between two trees, not with a reference"""
    if n in (9, 13):
        return family(n, count, m)
    t = np.linspace(0.0, 4.0, m)
    u = P.splitmix64_uniform(300 + n, count * (m + n)).reshape(count, m + n)
    data = 1.0 + 0.5 * np.exp(-t)[None, :] + np.exp(-0.5 * ((t[None, :] - 1.5 - 0.2 * u[:, :1]) / 0.4) ** 2) + 0.01 * (2 * u[:, n:] - 1)
    return t, data, 0.8 + 0.4 * u[:, :n]


def main(path):
    for i, m in enumerate(ROWS):
        for j, (n, dtype, model, has_grad) in enumerate([(3, np.float32, M.MODEL_EXP_DECAY, False), (3, np.float64, M.MODEL_EXP_DECAY, False),
                                                         (8, np.float32, M.MODEL_EXP_DECAY_PAD8, False),
                                                         (8, np.float64, M.MODEL_EXP_DECAY_PAD8, False),
                                                         (11, np.float64, M.MODEL16_GAUSS3_AFFINE, False),
                                                         (16, np.float64, M.MODEL16_EXP_HARM16, True)]):
            count = 4 + (i + j) % 5
            library_entries(n, dtype, model, has_grad, count, m, "n%d%s/m%d/count%d" % (n, PB.suffix(dtype), m, count))
            print("n = %d %s m = %d count = %d: done, %d arrays so far" % (n, PB.suffix(dtype), m, count, len(OUT)), flush=True)
    completion_by_the_general_solver()
    user_entries()
    # an .npz without time stamps: the same arrays give the same bytes
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(OUT):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, OUT[name], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name.replace("/", ".") + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    nonfinite = sum(int(np.count_nonzero(~np.isfinite(a))) for k, a in OUT.items() if a.dtype.kind == "f")
    print("%d arrays, %d values that are not finite, %d bytes, sha256 %s" % (len(OUT), nonfinite, os.path.getsize(path),
                                                                              hashlib.sha256(open(path, "rb").read()).hexdigest()))


if __name__ == "__main__":
    main(sys.argv[1])
