"""The batched one-wavefront-per-problem fit in double, measured (run on the GPU box from the repo root):
  * HIP-event time of ONE launch of mir_lsq_batched_kernel_d for 4096 problems at m = 512 -- PAD8 (n = 8) and EXP_DECAY (n = 3) --
    warmed up, median of REPS launches, next to mir_lsq_batched_kernel_s on the same problems (rounded to float);
  * the alternatives at that size, per fit: mir_optimize_least_squares_gpu_d looped over 64 of the problems (device callback of
    the same double model, launch_model_residual<ModelExpDecayPad8D>), and the f64 oracle over 64 problems (numpy callback);
  * the f64 launch alone (`one` argument: what the rocprofv3 kernel-trace / counter passes run, one launch after one warm-up).
Writes profiles/r07/batched_f64.txt (or prints only, with `one`)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mir_optim_amd as M                                                  # noqa: E402
from mir_optim_amd import api, build as hipbuild                           # noqa: E402
import test_gpu_batched_f64 as T                                           # noqa: E402  (the problem generators)

COUNT, MROWS, REPS = 4096, 512, 25


def launcher(model, dtype, x0, t, data):
    """returns launch() enqueuing one kernel-entry launch on torch's current stream from the same starts"""
    L = api.lib()
    suf = "d" if dtype == np.float64 else "s"
    count, n = x0.shape
    x0 = x0.astype(dtype)
    s = M.LeastSquaresSettings(dtype)
    b = [api.DeviceBuffer(a.astype(dtype)) for a in (t, data, x0, np.full(n, -np.inf), np.full(n, np.inf))]
    res = api.DeviceBuffer(nbytes=count * (32 if suf == "d" else 24), dtype=np.uint8, shape=(count * (32 if suf == "d" else 24),))
    basis = api.DeviceBuffer(nbytes=MROWS * 4 * np.dtype(dtype).itemsize, dtype=dtype, shape=(MROWS, 4))
    stream = torch.cuda.current_stream().cuda_stream
    opt = api.BatchedOptions(stream=stream, basis=basis.ptr, basis_bytes=basis.nbytes)
    fn = getattr(L, "mir_lsq_batched_kernel_" + suf)
    x0c = np.ascontiguousarray(x0)

    def launch():
        assert L.mir_lsq_memcpy_h2d(b[2].ptr, x0c.ctypes.data, x0c.nbytes, C.c_void_p(stream)) == 0
        rc = fn(C.byref(s), count, MROWS, model, b[2].ptr, b[3].ptr, b[4].ptr, b[0].ptr, 0, b[1].ptr, res.ptr, C.byref(opt))
        assert rc == 0, rc
    launch.keep = (b, res, basis)
    return launch


def kernel_only(model, dtype, x0, t, data):
    """launch() without the start upload: the kernel entry alone (x is overwritten by each fit; the problems of a repeated
    launch start where the last one stopped, so the timed launches upload the starts first, untimed)"""
    L = api.lib()
    full = launcher(model, dtype, x0, t, data)
    b, res, basis = full.keep
    suf = "d" if dtype == np.float64 else "s"
    s = M.LeastSquaresSettings(dtype)
    stream = torch.cuda.current_stream().cuda_stream
    opt = api.BatchedOptions(stream=stream, basis=basis.ptr, basis_bytes=basis.nbytes)
    fn = getattr(L, "mir_lsq_batched_kernel_" + suf)
    count = x0.shape[0]
    x0c = np.ascontiguousarray(x0.astype(dtype))

    def upload():
        assert L.mir_lsq_memcpy_h2d(b[2].ptr, x0c.ctypes.data, x0c.nbytes, C.c_void_p(stream)) == 0

    def run():
        rc = fn(C.byref(s), count, MROWS, model, b[2].ptr, b[3].ptr, b[4].ptr, b[0].ptr, 0, b[1].ptr, res.ptr, C.byref(opt))
        assert rc == 0, rc
    return upload, run, full


def timed(upload, run, reps):
    for _ in range(2):
        upload(); run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        upload()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def general_solver_per_fit(t, data, x0, k):
    UL = C.CDLL(hipbuild.user_model_f64_lib())
    fptr = C.cast(UL.user_pad8_residual_d, C.c_void_p).value

    class Ctx(C.Structure):
        _fields_ = [("t", C.c_void_p), ("data", C.c_void_p), ("stream", C.c_void_p)]
    L = api.lib()
    st = api.Stream()
    dt_ = api.DeviceBuffer(t)
    dd = [api.DeviceBuffer(data[i]) for i in range(k)]
    lo = np.full(8, -np.inf); up = np.full(8, np.inf)
    s = M.LeastSquaresSettings(np.float64)
    go = api.GpuOptions(flags=M.DEVICE_CALLBACKS, stream=st.handle)
    ctxs = [Ctx(dt_.ptr, dd[i].ptr, st.handle) for i in range(k)]

    def one(i):
        xg = x0[i].copy()
        r = L.mir_optimize_least_squares_gpu_d(C.byref(s), t.size, 8, xg.ctypes.data, lo.ctypes.data, up.ctypes.data,
                                               C.byref(go), C.addressof(ctxs[i]), fptr, None, None, None, None)
        assert r.status >= 0, r.status
    one(0)                                                   # warm-up (workspace, module loads)
    t0 = time.perf_counter()
    for i in range(k):
        one(i)
    return (time.perf_counter() - t0) / k


def oracle_per_fit(t, data, x0, k):
    from oracle import oracle as O
    O.build()
    t0 = time.perf_counter()
    for i in range(k):
        r, _ = T.oracle_fit(O, M.MODEL_EXP_DECAY_PAD8, t, data[i], x0[i])
        assert r.status >= 0
    return (time.perf_counter() - t0) / k


def main():
    torch.cuda.init()
    if len(sys.argv) > 1 and sys.argv[1] == "one":
        t, data, _, x0 = T.make_pad8(COUNT, MROWS)
        upload, run, _ = kernel_only(M.MODEL_EXP_DECAY_PAD8, np.float64, x0, t, data)
        upload(); run(); upload(); run()
        torch.cuda.synchronize()
        print("one f64 PAD8 launch of 4096 problems after a warm-up: done")
        return
    lines = [f"batched one-wavefront-per-problem fit, {COUNT} problems, m = {MROWS}; HIP events around ONE kernel-entry launch "
             f"(starts uploaded before, untimed), {REPS} launches after 2 warm-ups: median (min .. max)"]
    per_fit_d = None
    for model, name, maker in ((M.MODEL_EXP_DECAY_PAD8, "PAD8 (n = 8)", T.make_pad8), (M.MODEL_EXP_DECAY, "EXP_DECAY (n = 3)", T.make_exp_decay)):
        t, data, _, x0 = maker(COUNT, MROWS)
        row = {}
        for dtype in (np.float64, np.float32):
            upload, run, _ = kernel_only(model, dtype, x0, t, data)
            row[dtype] = timed(upload, run, REPS)
        d, s_ = row[np.float64], row[np.float32]
        lines.append(f"  {name:18s} f64 {d[0]:8.3f} ms ({d[1]:.3f} .. {d[2]:.3f})   f32 {s_[0]:8.3f} ms ({s_[1]:.3f} .. {s_[2]:.3f})"
                     f"   f64 / f32 = {d[0] / s_[0]:.2f}   f64 per fit {d[0] * 1e3 / COUNT:.3f} us")
        if model == M.MODEL_EXP_DECAY_PAD8:
            per_fit_d = d[0] * 1e-3 / COUNT
            tp, dp, xp = t, data, x0
    g = general_solver_per_fit(tp, dp, xp, 64)
    o = oracle_per_fit(tp, dp, xp, 64)
    lines.append(f"  PAD8 alternatives, per fit over 64 of the same problems: mir_optimize_least_squares_gpu_d (device callback "
                 f"of the same double model) {g * 1e3:.3f} ms; f64 oracle (numpy callback, one thread) {o * 1e3:.3f} ms")
    lines.append(f"  batched f64 per fit {per_fit_d * 1e6:.3f} us: {g / per_fit_d:.0f} x faster than the general solver, "
                 f"{o / per_fit_d:.0f} x faster than the oracle")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = os.path.join(ROOT, "profiles", "r07")
    os.makedirs(out, exist_ok=True)
    open(os.path.join(out, "batched_f64.txt"), "w").write(text)


if __name__ == "__main__":
    main()
