"""The batched one-wavefront-per-problem fit for models with 9 to 16 parameters, measured (run on the GPU from the repo root):
  * HIP-event time of ONE launch of mir_lsq_batched16_kernel_d for 4096 EXP_HARM16 fits (n = 16) at m = 512, warmed up,
    median of 25 launches (starts uploaded before each launch, untimed; caller-owned basis table, so the call is asynchronous);
  * the only way to run these fits before: mir_optimize_least_squares_gpu_d with a device callback of the same model
    (tests/user_model/user_model_n16.hip), looped over a 64-problem sample of the same fits, wall clock per problem;
  * for scale: one launch of the f64 EXP_DECAY_PAD8 batch (n = 8, mir_lsq_batched_kernel_d) at the same count and m.
Writes profiles/r14/batched16.txt (another directory: first argument)."""
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
import batched16_problems as PR                                            # noqa: E402  (tests/: the problem generators)

COUNT, MROWS, REPS, SAMPLE = 4096, 512, 25, 64


def kernel_launch(fn, model, nb, x0, t, data, extras):
    """(upload, run) for one kernel-entry launch on torch's current stream"""
    L = api.lib()
    count, n = x0.shape
    s = M.LeastSquaresSettings(np.float64)
    b = [api.DeviceBuffer(np.ascontiguousarray(a, dtype=np.float64)) for a in (t, data, x0, np.full(n, -np.inf), np.full(n, np.inf))]
    res = api.DeviceBuffer(nbytes=count * 32, dtype=np.uint8, shape=(count * 32,))
    basis = api.DeviceBuffer(nbytes=MROWS * nb * 8, dtype=np.float64, shape=(MROWS, nb))
    stream = torch.cuda.current_stream().cuda_stream
    opt = api.BatchedOptions(stream=stream, basis=basis.ptr, basis_bytes=basis.nbytes)
    x0c = np.ascontiguousarray(x0, dtype=np.float64)

    def upload():
        assert L.mir_lsq_memcpy_h2d(b[2].ptr, x0c.ctypes.data, x0c.nbytes, C.c_void_p(stream)) == 0

    def run():
        rc = fn(C.byref(s), count, MROWS, model, b[2].ptr, b[3].ptr, b[4].ptr, b[0].ptr, 0, b[1].ptr, res.ptr, C.byref(opt), *extras)
        assert rc == 0, rc

    def results():
        return np.frombuffer(res.download().tobytes(), dtype=PR.RDT).copy()
    run.keep = (b, res, basis, opt, s)
    return upload, run, results


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
    UL = C.CDLL(hipbuild.user_model_n16_lib())
    fptr = C.cast(UL.user_harm16_residual_d, C.c_void_p).value

    class Ctx(C.Structure):
        _fields_ = [("t", C.c_void_p), ("data", C.c_void_p), ("stream", C.c_void_p)]
    L = api.lib()
    st = api.Stream()
    n = x0.shape[1]
    dt_ = api.DeviceBuffer(np.ascontiguousarray(t))
    dd = [api.DeviceBuffer(np.ascontiguousarray(data[i])) for i in range(k)]
    lo = np.full(n, -np.inf); up = np.full(n, np.inf)
    s = M.LeastSquaresSettings(np.float64)
    go = api.GpuOptions(flags=M.DEVICE_CALLBACKS, stream=st.handle)
    ctxs = [Ctx(dt_.ptr, dd[i].ptr, st.handle) for i in range(k)]

    def one(i):
        xg = x0[i].copy()
        r = L.mir_optimize_least_squares_gpu_d(C.byref(s), t.size, n, xg.ctypes.data, lo.ctypes.data, up.ctypes.data,
                                               C.byref(go), C.addressof(ctxs[i]), fptr, None, None, None, None)
        assert r.status >= 0, r.status
    one(0)                                                   # warm-up (workspace, module loads)
    t0 = time.perf_counter()
    for i in range(k):
        one(i)
    return (time.perf_counter() - t0) / k


def main():
    torch.cuda.init()
    L = api.lib()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14")
    t, B, data, truth, x0 = PR.harm_problems(16, MROWS, COUNT)
    upload, run, results = kernel_launch(L.mir_lsq_batched16_kernel_d, M.MODEL16_EXP_HARM16, 13, x0, t, data, (None,))
    h = timed(upload, run, REPS)
    rec = results()
    assert np.all(rec["status"] >= 0), np.unique(rec["status"])
    t8, d8, x8 = PR.pad8_problems(COUNT, MROWS)
    up8, run8, _ = kernel_launch(L.mir_lsq_batched_kernel_d, M.MODEL_EXP_DECAY_PAD8, 4, x8, t8, d8, ())
    p = timed(up8, run8, REPS)
    g = general_solver_per_fit(t, data, x0, SAMPLE)
    per_fit = h[0] * 1e-3 / COUNT
    lines = [
        f"batched fits with 9 to 16 parameters (k_lm_batched16), {COUNT} problems, m = {MROWS}, f64; HIP events around ONE kernel-entry "
        f"launch (starts uploaded before, untimed), {REPS} launches after 2 warm-ups: median (min .. max)",
        f"  EXP_HARM16 (n = 16)     {h[0]:9.3f} ms ({h[1]:.3f} .. {h[2]:.3f})   per fit {per_fit * 1e6:8.3f} us   "
        f"iterations {rec['iterations'].mean():.1f}, residual evaluations {rec['fCalls'].mean():.1f} a fit (mean)",
        f"  EXP_DECAY_PAD8 (n = 8)  {p[0]:9.3f} ms ({p[1]:.3f} .. {p[2]:.3f})   per fit {p[0] * 1e3 / COUNT:8.3f} us   (mir_lsq_batched_kernel_d, for scale)",
        f"  mir_optimize_least_squares_gpu_d, device callback of the same 16-parameter model, {SAMPLE} of the same fits one by one: "
        f"{g * 1e3:.3f} ms per problem (wall clock)",
        (f"  the batched launch is {g / per_fit:.0f} x faster per fit than the general solver" if per_fit < g else
         f"  NO SPEED-UP: the batched launch takes {per_fit * 1e3:.3f} ms per fit, the general solver {g * 1e3:.3f} ms per problem"),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(out, exist_ok=True)
    open(os.path.join(out, "batched16.txt"), "w").write(text)


if __name__ == "__main__":
    main()
