"""The batched one-wavefront-per-problem fit for models with 9 to 16 parameters, measured (run on the GPU from the repo root):
  * HIP-event time of ONE launch of mir_lsq_batched16_kernel_d for 4096 EXP_HARM16 fits (n = 16) at m = 512, warmed up,
    median of 25 launches (starts uploaded before each launch, untimed; caller-owned basis table, so the call is asynchronous);
  * the only way to run these fits before: mir_optimize_least_squares_gpu_d with a device callback of the same model
    (tests/user_model/user_model_n16.hip), looped over a 64-problem sample of the same fits, wall clock per problem;
  * for scale: one launch of the f64 EXP_DECAY_PAD8 batch (n = 8, mir_lsq_batched_kernel_d) at the same count and m.
Writes profiles/r14/batched16.txt (another directory: first argument).

`python scripts/batched16.py weighted [directory]` measures weights and covariance at the same shape instead (4096 fits,
m = 512, n = 16): the unweighted launch of mir_lsq_batched16_kernel_d on the data of the first mode, twice (the figure of
profiles/r14 and the spread of two runs), then on the weighted set of tests/batched16_weighted_problems.py the unweighted
launch twice, the weighted launch of mir_lsq_batched16_kernel_ex_d, and the
covariance launch alone (mir_lsq_batched16_covariance_d on the weighted fit's records), with their ratios to the unweighted
launch. Writes profiles/r15/batched16_weighted_times.txt (another directory: second argument)."""
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


def kernel_launch(fn, model, nb, x0, t, data, extras, weights=None, covariance=False):
    """(upload, run) for one kernel-entry launch on torch's current stream. weights / covariance: the launch takes a
    mir_lsq_batched_extras with them (device buffers of this call) in place of `extras`"""
    L = api.lib()
    count, n = x0.shape
    s = M.LeastSquaresSettings(np.float64)
    b = [api.DeviceBuffer(np.ascontiguousarray(a, dtype=np.float64)) for a in (t, data, x0, np.full(n, -np.inf), np.full(n, np.inf))]
    res = api.DeviceBuffer(nbytes=count * 32, dtype=np.uint8, shape=(count * 32,))
    basis = api.DeviceBuffer(nbytes=MROWS * nb * 8, dtype=np.float64, shape=(MROWS, nb))
    stream = torch.cuda.current_stream().cuda_stream
    opt = api.BatchedOptions(stream=stream, basis=basis.ptr, basis_bytes=basis.nbytes)
    x0c = np.ascontiguousarray(x0, dtype=np.float64)
    dw = api.DeviceBuffer(np.ascontiguousarray(weights, dtype=np.float64)) if weights is not None else None
    dcov = api.DeviceBuffer(nbytes=count * n * n * 8, dtype=np.float64, shape=(count, n, n)) if covariance else None
    if dw is not None or dcov is not None:
        ex = api.BatchedExtras(weights=dw.ptr if dw else None, weight_stride=MROWS if dw else 0, covariance=dcov.ptr if dcov else None)
        extras = (C.byref(ex),)

    def upload():
        assert L.mir_lsq_memcpy_h2d(b[2].ptr, x0c.ctypes.data, x0c.nbytes, C.c_void_p(stream)) == 0

    def run():
        rc = fn(C.byref(s), count, MROWS, model, b[2].ptr, b[3].ptr, b[4].ptr, b[0].ptr, 0, b[1].ptr, res.ptr, C.byref(opt), *extras)
        assert rc == 0, rc

    def results():
        return np.frombuffer(res.download().tobytes(), dtype=PR.RDT).copy()
    run.keep = (b, res, basis, opt, s, dw, dcov, extras)
    run.cov = dcov
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


def weighted_main(out):
    import batched16_weighted_problems as WP16                             # tests/
    torch.cuda.init()
    L = api.lib()
    t, B, data, x0, w = WP16.harm_weighted(16, MROWS, COUNT)
    # the launch of main() on its own data (the figure of profiles/r14/batched16.txt), twice: the spread of two runs
    t14, _, data14, _, x14 = PR.harm_problems(16, MROWS, COUNT)
    base = kernel_launch(L.mir_lsq_batched16_kernel_d, M.MODEL16_EXP_HARM16, 13, x14, t14, data14, (None,))
    b1 = timed(base[0], base[1], REPS)
    plain = kernel_launch(L.mir_lsq_batched16_kernel_d, M.MODEL16_EXP_HARM16, 13, x0, t, data, (None,))
    u1 = timed(plain[0], plain[1], REPS)
    weighted = kernel_launch(L.mir_lsq_batched16_kernel_ex_d, M.MODEL16_EXP_HARM16, 13, x0, t, data, None, weights=w)
    wt = timed(weighted[0], weighted[1], REPS)
    u2 = timed(plain[0], plain[1], REPS)
    b2 = timed(base[0], base[1], REPS)
    rec_b, rec_u, rec_w = base[2](), plain[2](), weighted[2]()
    assert np.all(rec_b["status"] >= 0) and np.all(rec_u["status"] >= 0) and np.all(rec_w["status"] >= 0)
    # the covariance alone: the entry reads x and the records, so the weighted fit is made once and its x stays (no upload)
    cov = kernel_launch(L.mir_lsq_batched16_covariance_d, M.MODEL16_EXP_HARM16, 13, x0, t, data, None, weights=w, covariance=True)
    cov[0](); weighted_x = kernel_launch(L.mir_lsq_batched16_kernel_ex_d, M.MODEL16_EXP_HARM16, 13, x0, t, data, None, weights=w)
    weighted_x[0](); weighted_x[1](); torch.cuda.synchronize()
    xfit, rfit = weighted_x[1].keep[0][2].download(), weighted_x[1].keep[1].download()
    cov[1].keep[0][2].upload(xfit); cov[1].keep[1].upload(rfit)
    ct = timed(lambda: None, cov[1], REPS)
    c = cov[1].cov.download()
    assert np.isfinite(c).all()
    unw = min(u1[0], u2[0])
    lines = [
        f"weights and covariance of the batched fits with 9 to 16 parameters, {COUNT} EXP_HARM16 problems (n = 16), m = {MROWS}, f64; HIP "
        f"events around ONE kernel-entry launch (starts uploaded before, untimed), {REPS} launches after 2 warm-ups: median (min .. max)",
        f"  unweighted, the data of profiles/r14, first run    {b1[0]:9.3f} ms ({b1[1]:.3f} .. {b1[2]:.3f})   iterations {rec_b['iterations'].mean():.1f} a fit",
        f"  unweighted, the data of profiles/r14, second run   {b2[0]:9.3f} ms ({b2[1]:.3f} .. {b2[2]:.3f})   two runs differ by {abs(b1[0] / b2[0] - 1) * 100:.2f} %",
        "  on the heteroscedastic data of the weighted set:",
        f"  unweighted, mir_lsq_batched16_kernel_d, first run   {u1[0]:9.3f} ms ({u1[1]:.3f} .. {u1[2]:.3f})   iterations {rec_u['iterations'].mean():.1f} a fit",
        f"  unweighted, second run                             {u2[0]:9.3f} ms ({u2[1]:.3f} .. {u2[2]:.3f})   two runs differ by {abs(u1[0] / u2[0] - 1) * 100:.2f} %",
        f"  weighted, mir_lsq_batched16_kernel_ex_d            {wt[0]:9.3f} ms ({wt[1]:.3f} .. {wt[2]:.3f})   {wt[0] / unw:.3f} x the unweighted launch; "
        f"iterations {rec_w['iterations'].mean():.1f} a fit (another objective)",
        f"  covariance alone, mir_lsq_batched16_covariance_d   {ct[0]:9.3f} ms ({ct[1]:.3f} .. {ct[2]:.3f})   {ct[0] / unw:.3f} x the unweighted launch; "
        f"per problem {ct[0] * 1e3 / COUNT:.3f} us",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(out, exist_ok=True)
    open(os.path.join(out, "batched16_weighted_times.txt"), "w").write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "weighted":
        weighted_main(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r15"))
    else:
        main()
