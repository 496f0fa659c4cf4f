"""What per-row weights and the covariance kernel cost on the batched path (run on the GPU box from the repo root, one
precision per process: scripts/batched_weighted_cost.sh chains the two under a time limit each):
HIP-event time of ONE launch for 4096 PAD8 problems (m = 512, n = 8), warmed up, median of REPS launches from the same starts,
  * mir_lsq_batched_kernel_ex_{s,d} without extras (the unweighted instance), with per-problem weights, and with weights of
    ones (the same trajectory as the unweighted fit: the cost of the instance alone, not of other iterates),
  * mir_lsq_batched_covariance_{s,d} alone on the results of the weighted fit.
Prints one line per figure; the start upload is enqueued before the first event and is not timed."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mir_optim_amd as M                                                  # noqa: E402
from mir_optim_amd import api                                              # noqa: E402
import weighted_problems as WP                                             # noqa: E402

COUNT, MROWS, N, REPS = 4096, 512, 8, 15


def main(name):
    dtype = {"f32": np.float32, "f64": np.float64}[name]
    suf = "s" if dtype == np.float32 else "d"
    L = api.lib()
    t, data, x0, w = [np.ascontiguousarray(a, dtype=dtype) for a in WP.pad8_weighted(COUNT, MROWS)]
    s = M.LeastSquaresSettings(dtype)
    item = np.dtype(dtype).itemsize
    lo, up = np.full(N, -np.inf, dtype), np.full(N, np.inf, dtype)
    dt_, dd, dx, dlo, dup, dw = [api.DeviceBuffer(a) for a in (t, data, x0, lo, up, w)]
    done = api.DeviceBuffer(np.ones_like(w))
    rec = 24 if suf == "s" else 32
    dres = api.DeviceBuffer(nbytes=COUNT * rec, dtype=np.uint8, shape=(COUNT * rec,))
    dbasis = api.DeviceBuffer(nbytes=MROWS * 4 * item, dtype=dtype, shape=(MROWS, 4))
    dcov = api.DeviceBuffer(nbytes=COUNT * N * N * item, dtype=dtype, shape=(COUNT, N, N))
    stream = torch.cuda.current_stream().cuda_stream
    opt = api.BatchedOptions(stream=stream, basis=dbasis.ptr, basis_bytes=dbasis.nbytes)
    fit = getattr(L, "mir_lsq_batched_kernel_ex_" + suf)
    covfn = getattr(L, "mir_lsq_batched_covariance_" + suf)
    args = [C.byref(s), COUNT, MROWS, M.MODEL_EXP_DECAY_PAD8, dx.ptr, dlo.ptr, dup.ptr, dt_.ptr, 0, dd.ptr, dres.ptr, C.byref(opt)]

    def timed(fn, extras, upload):
        ms = []
        for rep in range(REPS + 3):
            if upload:
                assert L.mir_lsq_memcpy_h2d(dx.ptr, x0.ctypes.data, x0.nbytes, C.c_void_p(stream)) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args, C.byref(extras) if extras is not None else None)
            e1.record()
            assert rc == 0, rc
            torch.cuda.synchronize()
            if rep >= 3:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    def line(label, r):
        print(f"{name} {label:<46s} median {r[0]:8.3f} ms  (min {r[1]:.3f}, max {r[2]:.3f}; {REPS} launches)  "
              f"{r[0] * 1e3 / COUNT:.3f} us / problem", flush=True)

    line("fit, no extras (unweighted instance)", timed(fit, None, True))
    line("fit, weights of ones (weighted instance)", timed(fit, api.BatchedExtras(weights=done.ptr, weight_stride=MROWS), True))
    line("fit, weights 1 / sigma (other iterates)", timed(fit, api.BatchedExtras(weights=dw.ptr, weight_stride=MROWS), True))
    wcov = api.BatchedExtras(weights=dw.ptr, weight_stride=MROWS, covariance=dcov.ptr)
    line("fit + covariance, weights 1 / sigma", timed(fit, wcov, True))
    line("covariance kernel alone (weighted, FD)", timed(covfn, wcov, False))
    raw = np.frombuffer(dres.download().tobytes(), dtype=np.dtype([("status", "<i4"), ("it", "<u4"), ("f", "<u4"), ("g", "<u4"),
                                                                    ("r", dtype), ("l", dtype)]))
    cov = dcov.download()
    print(f"{name} statuses >= 0: {(raw['status'] >= 0).all()}, iterations {raw['it'].sum()}, fCalls {raw['f'].sum()}, "
          f"finite covariance: {np.isfinite(cov).all()}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
