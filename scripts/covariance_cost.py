#!/usr/bin/env python
"""What the covariance step costs on the GPU (writes profiles/r09/covariance.txt).

  1. the SPD inverse alone (mir_lsq_spd_inverse_work_*: two launches, caller-owned scratch, no allocation or synchronisation
     inside) at n = 16, 128, 256, 1024 in f64 and n = 128 in f32: HIP events around the call on one stream, after warm-up calls,
     minimum and median over the repetitions; with the accuracy of each result against numpy;
  2. the whole mir_lsq_covariance_gpu_d call at cfg 3's shape (m = 1e6 x n = 128, device callbacks with the difference panel,
     the solve's workspace): host clock around the call (it ends in a device synchronise) and the solver's own HIP-event
     brackets (mir_lsq_stats: fd_callback_ms, jtj_fd_ms) -- beside one solve at the same shape in the same process, whose
     refresh round (fd_callback_ms + jtj_fd_ms per full refresh) is what the call contains, plus the inverse.

Needs an MI355X; there is no CPU path.  python scripts/covariance_cost.py [--rows 1000000] [--out profiles/r09/covariance.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spd(n, seed, cond=1e3):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * np.geomspace(1.0, cond, n)) @ Q.T


def time_inverse(M, api, torch, n, dtype, reps, warm=5):
    L = api.lib()
    suf = "d" if dtype == np.float64 else "s"
    P = spd(n, n)
    dP = api.DeviceBuffer(P.astype(dtype))
    dX = api.DeviceBuffer(nbytes=n * n * np.dtype(dtype).itemsize, dtype=dtype, shape=(n, n))
    di = api.DeviceBuffer(nbytes=4, dtype=np.int32, shape=(1,))
    wb = L.mir_lsq_spd_inverse_work_bytes(n, np.dtype(dtype).itemsize)
    dW = api.DeviceBuffer(nbytes=wb, dtype=np.uint8, shape=(wb,))
    stream = torch.cuda.Stream()
    fn = getattr(L, "mir_lsq_spd_inverse_work_" + suf)
    ms = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = fn(n, dP.ptr, None, dX.ptr, di.ptr, dW.ptr, wb, C.c_void_p(stream.cuda_stream))
        e1.record(stream)
        stream.synchronize()
        if rc != 0:
            raise SystemExit(f"mir_lsq_spd_inverse_work_{suf} failed: {rc}")
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    X = dX.download().astype(np.float64)
    Xr = np.linalg.inv(P)
    err = np.abs(X - Xr).max() / np.abs(Xr).max()
    nres = np.linalg.norm(P.astype(dtype).astype(np.float64) @ X - np.eye(n)) / (np.linalg.norm(P) * np.linalg.norm(X))
    for b in (dP, dX, di, dW):
        b.free()
    return min(ms) * 1e3, statistics.median(ms) * 1e3, err, nres


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "covariance.txt"))
    args = ap.parse_args()
    import torch

    import mir_optim_amd as M
    from mir_optim_amd import api, workloads as W
    if not torch.cuda.is_available() or M.device_count() < 1:
        raise SystemExit("covariance_cost.py needs a GPU: mir_optim_amd has no CPU path")
    lines = [f"covariance step on {torch.cuda.get_device_name(0)}; {api.lib().mir_lsq_version().decode()}", ""]
    lines.append("SPD inverse alone (k_spd_factor + k_spd_columns, HIP events around the call that enqueues the two launches, "
                 f"{args.reps} repetitions after 5 warm-up calls; the bracket includes the host's enqueue of the two launches, "
                 "~10-20 us, which dominates at n = 16)")
    lines.append(f"{'dtype':8}{'n':>6}{'min us':>12}{'median us':>12}{'err vs numpy':>16}{'nres':>12}")
    for dtype, n in [(np.float64, 16), (np.float64, 128), (np.float64, 256), (np.float64, 1024), (np.float32, 128)]:
        mn, med, err, nres = time_inverse(M, api, torch, n, dtype, args.reps)
        lines.append(f"{np.dtype(dtype).name:8}{n:>6}{mn:>12.1f}{med:>12.1f}{err:>16.3e}{nres:>12.3e}")
    lines.append("")

    m, n = args.rows, args.n
    data = W.tanh_linear_data(m, n)
    prob = W.TanhLinear(data["A"], data["b"])
    ws = api.lib().mir_lsq_workspace_create(m, n, 8)
    if not ws:
        raise SystemExit("workspace allocation failed")
    s = M.LeastSquaresSettings()
    s.absTolerance = 1e-5
    for _ in range(2):                                                   # warm-up: code objects, the FD panel allocation
        res, x = prob.solve(data["x0"], settings=s, batched=True, workspace=ws)
    st = M.Stats()
    t0 = time.perf_counter()
    res, x = prob.solve(data["x0"], settings=s, batched=True, workspace=ws, stats=st, flags=M.TIME_KERNELS)
    solve_ms = (time.perf_counter() - t0) * 1e3
    refresh_ms = (st.fd_callback_ms + st.jtj_fd_ms) / max(1, st.jacobian_full)

    def cov_call(stats=None, flags=0):
        opts = prob.options(batched=True, workspace=ws, stats=stats, flags=flags)
        t = time.perf_counter()
        out = M.covariance(prob.f, m, x, options=opts, fContext=C.addressof(prob.ctx))
        return (time.perf_counter() - t) * 1e3, out
    for _ in range(2):
        cov_call()
    wall = [cov_call()[0] for _ in range(args.calls)]
    sc = M.Stats()
    wall_t, (cov, se, rr, info) = cov_call(stats=sc, flags=M.TIME_KERNELS)
    lines += [f"whole call at m = {m} x n = {n}, f64, device callbacks with the difference panel, the solve's workspace",
              f"  one solve (absTolerance 1e-5): {solve_ms:.3f} ms wall, {res.iterations} iterations, {st.jacobian_full} full refresh(es), "
              f"status {res.status.name}",
              f"  one full-refresh round of that solve (HIP events): fd callbacks {st.fd_callback_ms / max(1, st.jacobian_full):.3f} ms + "
              f"fd J^T J kernel {st.jtj_fd_ms / max(1, st.jacobian_full):.3f} ms = {refresh_ms:.3f} ms",
              f"  mir_lsq_covariance_gpu_d, HOST CLOCK (not HIP events; the call ends in a device synchronise) over {args.calls} calls: min {min(wall):.3f} ms, median {statistics.median(wall):.3f} ms",
              f"  ... its own brackets (one call with TIME_KERNELS, {wall_t:.3f} ms wall): fd callbacks {sc.fd_callback_ms:.3f} ms + "
              f"fd J^T J kernel {sc.jtj_fd_ms:.3f} ms = {sc.fd_callback_ms + sc.jtj_fd_ms:.3f} ms; the rest is f(x), ||f||^2, the inverse, "
              f"the scale, the copy of {n} x {n} and the host side",
              f"  info {info}, residual {rr:.6e}, largest standard error {np.max(se):.3e}, library launches {sc.library_launches}", ""]
    api.lib().mir_lsq_workspace_destroy(ws)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
