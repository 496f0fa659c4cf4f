"""The fitted-curve / confidence-band kernel (k_batched_predict, csrc/batched_predict.h) measured on the GPU box, from the repo root:

  python scripts/batched_predict.py gaps    the worst gap of every comparison tests/test_gpu_batched_predict.py makes, per
                                            (family, precision, kind), beside the CPU figure of tests/predict_cases.py and the bar
                                            that follows from the two (10 x the larger, rounded up to one digit): the table of
                                            that test's docstring. The test functions themselves are run, with their `check`
                                            recording instead of asserting; their bit-for-bit identities still assert.
  python scripts/batched_predict.py time    HIP-event time of ONE launch for 4096 problems x q = 512 (warmed up, median of 15):
                                            PAD8 in f32 and f64 with and without sigma (central differences), EXP_HARM16 by
                                            central differences and by its gradient; the covariance kernel on the same batch
                                            (m = 512) for comparison; and the time the 2 count q output values take at the
                                            6.0 TB/s DESIGN.md quotes for plain stores.
profiles/r25/batched_predict.txt holds the output of both."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mir_optim_amd as M                                                  # noqa: E402
from mir_optim_amd import api                                              # noqa: E402
import predict_cases as PC                                                 # noqa: E402

COUNT, Q, MROWS, REPS = 4096, 512, 512, 15
STORE_RATE = 6.0e12


def gaps():
    import test_gpu_batched_predict as T
    worst = {}

    def record(inst, kind, v, s, ref, label):
        fam, dtype = T.INSTANCES[inst][0], np.dtype(T.INSTANCES[inst][1]).name
        vr, sr, mag = ref
        assert np.isfinite(v).all() and np.isfinite(s).all()
        for key, g in (((fam, dtype, "value"), PC.value_gap(v, vr)), ((fam, dtype, kind), PC.sigma_gap(s, sr, mag))):
            worst[key] = max(worst.get(key, 0.0), g)
        print(f"  {fam} {dtype} {label}: value {PC.value_gap(v, vr):.3e}  sigma {kind} {PC.sigma_gap(s, sr, mag):.3e}", flush=True)

    T.check = record
    for inst in T.BUILTIN8:
        for q in PC.QS:
            T.test_builtin_models_value_and_band_by_central_differences(inst, q)
    for inst, variant in (("harm16", 0), ("harm16", T.ANALYTIC), ("gauss3", 0)):
        T.test_wide_builtin_models(inst, variant)
    for inst in ("peak-f32", "peak-f64", "harm13"):
        T.test_the_user_library(inst)
    for inst in ("exp_decay-f32", "pad8-f32", "pad8-f64", "harm16", "peak-f64"):
        T.test_fixed_parameters_and_clipped_differences(inst)
    for inst in T.END_TO_END:
        T.test_end_to_end_fit_covariance_predict_on_device_buffers(inst)
    print(f"{'family':<10s} {'precision':<8s} {'kind':<9s} {'CPU figure':>11s} {'measured':>11s} {'bar':>8s}")
    for (fam, dtype, kind), g in sorted(worst.items()):
        print(f"{fam:<10s} {dtype:<8s} {kind:<9s} {PC.CPU_FIGURE[(fam, dtype)][kind]:11.1e} {g:11.2e} {PC.bar(fam, dtype, kind, g):8.0e}")
    print("DEVICE_GAP = {")
    for (fam, dtype, kind), g in sorted(worst.items()):
        print(f"    ({fam!r}, {dtype!r}, {kind!r}): {g:.2e},")
    print("}")


def time_launches():
    import torch
    L = api.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(call):
        ms = []
        for rep in range(REPS + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = call()
            e1.record()
            assert rc == 0, rc
            torch.cuda.synchronize()
            if rep >= 3:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    def line(label, r):
        print(f"{label:<58s} median {r[0] * 1e3:9.1f} us  (min {r[1] * 1e3:.1f}, max {r[2] * 1e3:.1f}; {REPS} launches)", flush=True)

    for name, dtype, famname, model, entry, coventry in (
            ("PAD8 f32", np.float32, "pad8", M.MODEL_EXP_DECAY_PAD8, "mir_lsq_batched_predict_s", "mir_lsq_batched_covariance_s"),
            ("PAD8 f64", np.float64, "pad8", M.MODEL_EXP_DECAY_PAD8, "mir_lsq_batched_predict_d", "mir_lsq_batched_covariance_d"),
            ("EXP_HARM16 f64", np.float64, "harm16", M.MODEL16_EXP_HARM16, "mir_lsq_batched16_predict_d", "mir_lsq_batched16_covariance_d")):
        fam = PC.family(famname)
        n, item = fam.n, np.dtype(dtype).itemsize
        reps = COUNT // PC.COUNT
        x = np.tile(fam.x, (reps, 1)).astype(dtype); cov = np.tile(fam.C, (reps, 1, 1)).astype(dtype)
        tq = np.linspace(-0.25, 4.25, Q).astype(dtype)
        s = M.LeastSquaresSettings(dtype)
        dx, dtq, dcov = [api.DeviceBuffer(a) for a in (x, tq, cov)]
        dv, ds = [api.DeviceBuffer(nbytes=COUNT * Q * item, dtype=dtype, shape=(COUNT, Q)) for _ in range(2)]
        fn = getattr(L, entry)

        def call(sigma, variant=0):
            opt = api.BatchedOptions(stream=stream, variant=variant)
            return fn(C.byref(s), COUNT, Q, model, dx.ptr, None, None, dtq.ptr, 0, dcov.ptr if sigma else None, dv.ptr,
                      ds.ptr if sigma else None, C.byref(opt), None)

        line(f"{name}: value only", timed(lambda: call(False)))
        line(f"{name}: value + sigma, central differences", timed(lambda: call(True)))
        if famname == "harm16":
            line(f"{name}: value + sigma, the model's gradient", timed(lambda: call(True, 2)))
        v, sg = dv.download(), ds.download()
        assert np.isfinite(v).all() and np.isfinite(sg).all() and (sg > 0).all()
        # the covariance kernel on the same batch: m = 512 rows at t = linspace(0, 4), records of a finished fit made by hand
        t = np.linspace(0.0, 4.0, MROWS).astype(dtype)
        data = np.stack([fam.value(t.astype(np.float64), fam.x[k]) for k in range(PC.COUNT)])
        data = np.tile(data, (reps, 1)).astype(dtype)
        R = np.dtype([("status", "<i4"), ("it", "<u4"), ("f", "<u4"), ("g", "<u4"), ("r", dtype), ("l", dtype)])
        recs = np.zeros(COUNT, dtype=R); recs["status"] = 1; recs["r"] = 1.0
        lo, up = np.full(n, -np.inf, dtype), np.full(n, np.inf, dtype)
        dt_, dd, dlo, dup, dres = [api.DeviceBuffer(a) for a in (t, data, lo, up, recs.view(np.uint8))]
        nb = {"pad8": 4, "harm16": 13}[famname]
        dbasis = api.DeviceBuffer(nbytes=MROWS * nb * item, dtype=dtype, shape=(MROWS, nb))
        dcov2 = api.DeviceBuffer(nbytes=COUNT * n * n * item, dtype=dtype, shape=(COUNT, n, n))
        ex = api.BatchedExtras(covariance=dcov2.ptr)
        opt = api.BatchedOptions(stream=stream, basis=dbasis.ptr, basis_bytes=dbasis.nbytes)
        cfn = getattr(L, coventry)
        line(f"{name}: covariance kernel, m = {MROWS}, central differences",
             timed(lambda: cfn(C.byref(s), COUNT, MROWS, model, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, 0, dd.ptr, dres.ptr, C.byref(opt),
                               C.byref(ex))))
        assert np.isfinite(dcov2.download()).all()
        print(f"{name}: 2 x {COUNT} x {Q} output values = {2 * COUNT * Q * item / 1e6:.1f} MB: "
              f"{2 * COUNT * Q * item / STORE_RATE * 1e6:.1f} us at {STORE_RATE / 1e12:.1f} TB/s", flush=True)
        for b in (dx, dtq, dcov, dv, ds, dt_, dd, dlo, dup, dres, dbasis, dcov2):
            b.free()


if __name__ == "__main__":
    {"gaps": gaps, "time": time_launches}[sys.argv[1]]()
