"""Time of one batched BOXCQP launch (four problems a wave; --n 8: mir_lsq_batched_box_qp_s / _d, csrc/boxqp_rows.h; --n 16:
mir_lsq_batched_box_qp16_s / _d, one matrix row per lane, csrc/boxqp_rows16.h; --n 32 and --n 64: mir_lsq_batched_box_qp64_s /
_d, two problems or one a wave with the matrices in LDS, csrc/boxqp_wave.h, dense layout) against the only way there was before
it, a loop over the one-problem host-pointer entry mir_solve_box_qp_gpu_*.

65 536 problems of order n = 8 or 16 (16 384 of order 32 or 64: A alone is 2.3 GB of host memory at 65 536 x 68 x 64),
P = A^T A / m + 0.05 I (A m x n standard normal, m = n + 4), q = 2 N(0, 1), bounds c -+ w with c ~ N(0, 1), w ~ U(0.5, 3):
about half the variables end on a bound (the share is printed). float32 and float64.
  * batched: device events around `reps` launches on one stream after a warm-up, the median per launch; operands resident.
  * loop: a host clock around a loop over the first 256 problems (each call allocates, copies in, launches, synchronises and
    copies out: that is the entry), per problem, extrapolated to the full count.
Run from the repository root:  timeout 300 python scripts/probes/batched_boxqp.py --n {8,16,32,64} [--out FILE]
(profiles/r10/batched_boxqp.txt and profiles/r11/batched_boxqp16.txt are the first records at n = 8 and n = 16,
profiles/r29/batched_boxqp_n32.txt and batched_boxqp_n64.txt at n = 32 and n = 64)
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import mir_optim_amd as M          # noqa: E402
from mir_optim_amd import api      # noqa: E402

COUNT, SAMPLE = 65536, 256            # main() takes 16 384 problems at n > 16


def problems(N, dtype, seed=10):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((COUNT, N + 4, N))
    P = np.einsum("pki,pkj->pij", A, A) / (N + 4) + 0.05 * np.eye(N)
    q = 2 * rng.standard_normal((COUNT, N))
    c, w = rng.standard_normal((COUNT, N)), rng.uniform(0.5, 3.0, (COUNT, N))
    return tuple(a.astype(dtype) for a in (P, q, c - w, c + w))


def batched_ms(N, dtype, P, q, l, u, reps=50):
    W = 8 if N <= 8 else 16 if N <= 16 else N                  # the layout's width: operands are padded to it (n > 16: dense)
    fn = getattr(api.lib(), "mir_lsq_batched_box_qp" + ("" if W == 8 else "16" if W == 16 else "64") + ("_s" if dtype == np.float32 else "_d"))
    dev = torch.device("cuda")
    pad = lambda a, shape: torch.from_numpy(np.pad(a, [(0, 0)] + [(0, W - N)] * (a.ndim - 1))).to(dev).reshape(shape).contiguous()
    dP, dq, dl, du = pad(P, (COUNT, W * W)), pad(q, (COUNT, W)), pad(l, (COUNT, W)), pad(u, (COUNT, W))
    dx = torch.zeros((COUNT, W), dtype=dP.dtype, device=dev)
    dst = torch.zeros(COUNT, dtype=torch.int32, device=dev)
    dit = torch.zeros(COUNT, dtype=torch.int32, device=dev)
    s = M.BoxQPSettings(dtype)
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        rc = fn(C.addressof(s), COUNT, N, dP.data_ptr(), dq.data_ptr(), dl.data_ptr(), du.data_ptr(), W, dx.data_ptr(),
                dst.data_ptr(), dit.data_ptr(), 0, stream)
        assert rc == 0, rc
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); launch(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    x, st, it = dx.cpu().numpy()[:, :N], dst.cpu().numpy(), dit.cpu().numpy()
    return ts[len(ts) // 2], ts[0], ts[-1], x, st, it


def loop_ms_per_problem(dtype, P, q, l, u):
    for p in range(8):                                         # warm-up: code objects, allocator
        M.solveBoxQP(np.tril(P[p]), q[p], l[p], u[p], dtype=dtype)
    t0 = time.perf_counter()
    out = [M.solveBoxQP(np.tril(P[p]), q[p], l[p], u[p], dtype=dtype) for p in range(SAMPLE)]
    dt = (time.perf_counter() - t0) * 1e3 / SAMPLE
    return dt, np.stack([o[1] for o in out]), np.array([int(o[0]) for o in out]), np.array([o[2] for o in out])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, choices=(8, 16, 32, 64), default=8)
    ap.add_argument("--out", default=None, help="default: profiles/r12/batched_boxqp_n<N>.txt (n > 16: profiles/r29)")
    args = ap.parse_args()
    N = args.n
    global COUNT
    COUNT = 65536 if N <= 16 else 16384
    out = args.out or os.path.join("profiles", "r12" if N <= 16 else "r29", "batched_boxqp_n%d.txt" % N)
    lines = [f"batched BOXCQP on {torch.cuda.get_device_name(0)}; {api.lib().mir_lsq_version().decode()}",
             f"{COUNT} problems, n = {N}; loop baseline on the first {SAMPLE}, extrapolated", ""]
    for dtype in (np.float32, np.float64):
        P, q, l, u = problems(N, dtype)
        med, lo, hi, x, st, it = batched_ms(N, dtype, P, q, l, u)
        per, xl, stl, itl = loop_ms_per_problem(dtype, P, q, l, u)
        active = float(np.mean((x == l) | (x == u)))
        agree = int(np.sum((st[:SAMPLE] == stl) & (it[:SAMPLE] == itl)))
        lines += [f"{np.dtype(dtype).name}:",
                  f"  batched launch        {med:9.4f} ms median of 50 (min {lo:.4f}, max {hi:.4f}) = {med * 1e6 / COUNT:.1f} ns a problem",
                  f"  loop over one-problem entry  {per:9.4f} ms a problem on {SAMPLE} -> {per * COUNT:.0f} ms for {COUNT} (extrapolated)",
                  f"  ratio                 {per * COUNT / med:9.0f} x",
                  f"  status counts (solved, numericError, maxIterations) {np.bincount(st, minlength=3).tolist()}; "
                  f"mean iterations {it.mean():.2f}, max {it.max()}; variables on a bound {active:.2f}",
                  f"  status and iterations equal to the loop's on {agree} of {SAMPLE}; "
                  f"max |x - x_loop| {np.max(np.abs(x[:SAMPLE].astype(np.float64) - xl)):.3e}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
