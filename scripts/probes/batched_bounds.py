"""What the in-kernel bounded step of the batched fit costs (MIR_LSQ_BATCHED_DEVICE_BOUNDS, csrc/batched_bounded.h).

4096 problems of the B8 formulas of tests/test_gpu_batched_bounds.py (MODEL_EXP_DECAY_PAD8, seeds 900 + k, m = 512), float32 and
float64, one kernel-entry launch (mir_lsq_batched_kernel_s / _d) on resident operands with a caller-owned basis table:
  (a) the bounded instance with B8's box          (b) the bounded instance with infinite bounds
  (c) the default instance with infinite bounds   (the kernel every unbounded fit runs; its code is the parent's)
  (d) the parent's way for the bounded batch: the host entry WITHOUT the bit (the general solver finishes every -100 problem,
      one at a time) on the first 64 problems, host clock, extrapolated to 4096.
(a), (b), (c): device events around ONE launch, alternating a, b, c within a repetition, the median of 25 after 3 warm-ups each.
Ratios: (a)/(c) the price of bounds, (b)/(c) the price of carrying the unused code, (d)/(a).
Run from the repository root:  timeout 600 python scripts/probes/batched_bounds.py [--out FILE] [--only a --dtype f32 --reps N]
(--only: just that variant, no file written -- for a counter pass of its own:
   rocprofv3 --pmc VALUBusy -d DIR -- python scripts/probes/batched_bounds.py --only a --dtype f32 --reps 3)
profiles/r13/batched_bounds.txt is the first record.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mir_optim_amd as M          # noqa: E402
from mir_optim_amd import api      # noqa: E402
import problems as P               # noqa: E402

COUNT, SAMPLE, MROWS = 4096, 64, 512
LOWER = np.array([-np.inf, 1.0, 0.0, -0.1, -0.1, -0.1, -0.1, -np.inf])
UPPER = np.array([np.inf, 2.0, np.inf, 0.1, 0.1, 0.1, 0.1, np.inf])


def problems(count, m):
    t = np.linspace(0.0, 4.0, m)
    basis = np.stack([np.sin(2 * t), np.cos(2 * t), np.sin(5 * t), np.cos(5 * t), t])
    data = np.empty((count, m)); x0 = np.empty((count, 8))
    for k in range(count):
        u = P.splitmix64_uniform(900 + k, m + 16)
        p = np.array([1.0 + u[0], 0.5 + 2.0 * u[1], 0.2 * u[2], 0.6 * u[3] - 0.3, 0.6 * u[4] - 0.3, 0.6 * u[5] - 0.3,
                      0.6 * u[6] - 0.3, 0.1 * u[7] - 0.05])
        data[k] = p[0] * np.exp(-t * p[1]) + p[2] + p[3:] @ basis + 0.01 * (2 * u[16:] - 1)
        x0[k] = p
        x0[k, :2] *= 1 + 0.2 * (2 * u[8:10] - 1)
        x0[k, 2:] += 0.1 * (2 * u[10:16] - 1)
    return t, data, x0


class Launcher:
    """one variant of the kernel-entry launch on resident data"""

    def __init__(self, dtype, t, data, x0, lo, up, variant):
        dev = torch.device("cuda")
        tt = torch.float32 if dtype == np.float32 else torch.float64
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
        self.t, self.data, self.x0, self.lo, self.up = to(t), to(data), to(x0), to(lo), to(up)
        self.x = self.x0.clone()
        self.count, self.m = data.shape
        rec = 24 if dtype == np.float32 else 32
        self.res = torch.zeros(self.count * rec, dtype=torch.uint8, device=dev)
        self.basis = torch.zeros((self.m, 4), dtype=tt, device=dev)
        self.s = M.LeastSquaresSettings(dtype)
        self.fn = getattr(api.lib(), "mir_lsq_batched_kernel_" + ("s" if dtype == np.float32 else "d"))
        self.opt = api.BatchedOptions(stream=torch.cuda.current_stream().cuda_stream, basis=self.basis.data_ptr(),
                                      basis_bytes=self.basis.numel() * self.basis.element_size(), variant=variant)
        self.rdt = np.dtype([("status", "<i4"), ("iterations", "<u4"), ("fCalls", "<u4"), ("gCalls", "<u4"),
                             ("residual", "<f4" if dtype == np.float32 else "<f8"), ("lambda", "<f4" if dtype == np.float32 else "<f8")])

    def timed(self):
        self.x.copy_(self.x0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = self.fn(C.byref(self.s), self.count, self.m, M.MODEL_EXP_DECAY_PAD8, self.x.data_ptr(), self.lo.data_ptr(),
                     self.up.data_ptr(), self.t.data_ptr(), 0, self.data.data_ptr(), self.res.data_ptr(), C.byref(self.opt))
        e1.record()
        assert rc == 0, rc
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def records(self):
        return np.frombuffer(self.res.cpu().numpy().tobytes(), dtype=self.rdt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "batched_bounds.txt"))
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    ap.add_argument("--dtype", choices=("f32", "f64"), default=None)
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    t, data, x0 = problems(COUNT, MROWS)
    x0b = np.clip(x0, LOWER, UPPER)
    inf = np.full(8, np.inf)
    lines = [f"batched fits with in-kernel bounded steps on {torch.cuda.get_device_name(0)}; {api.lib().mir_lsq_version().decode()}",
             f"{COUNT} problems of B8's formulas, m = {MROWS}, n = 8; device events around one launch, median of {args.reps}", ""]
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        if args.dtype and args.dtype != name:
            continue
        L = {"a": Launcher(dtype, t, data, x0b, LOWER, UPPER, M.BATCHED_DEVICE_BOUNDS),
             "b": Launcher(dtype, t, data, x0b, -inf, inf, M.BATCHED_DEVICE_BOUNDS),
             "c": Launcher(dtype, t, data, x0b, -inf, inf, 0)}
        keys = [args.only] if args.only else ["a", "b", "c"]
        for k in keys:
            for _ in range(3):
                L[k].timed()
        ts = {k: [] for k in keys}
        for _ in range(args.reps):
            for k in keys:
                ts[k].append(L[k].timed())
        med = {k: float(np.median(v)) for k, v in ts.items()}
        lines.append(f"{np.dtype(dtype).name}:")
        label = {"a": "(a) bounded instance, B8's box      ", "b": "(b) bounded instance, infinite box  ", "c": "(c) default instance, infinite box  "}
        for k in keys:
            r = L[k].records()
            lines.append(f"  {label[k]} {med[k]:9.4f} ms (min {min(ts[k]):.4f}, max {max(ts[k]):.4f}) = {med[k] * 1e3 / COUNT:.3f} us a fit; "
                         f"statuses {dict(zip(*[a.tolist() for a in np.unique(r['status'], return_counts=True)]))}, "
                         f"mean iterations {r['iterations'].mean():.2f}, mean fCalls {r['fCalls'].mean():.1f}")
        if args.only:
            continue
        rb, rc = L["b"].records(), L["c"].records()
        lines.append(f"  (b) and (c) return the same bits: {rb.tobytes() == rc.tobytes() and bool(torch.equal(L['b'].x, L['c'].x))}")
        xa = L["a"].x.cpu().numpy()
        on = (xa == LOWER.astype(dtype)) | (xa == UPPER.astype(dtype))
        lines.append(f"  (a): parameters on a bound per problem, histogram {np.bincount(on.sum(axis=1)).tolist()}")
        # (d): the host entry without the bit on a sample (its general-solver fallback runs for every -100 problem)
        M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY_PAD8, x0b[:4], t, data[:4], l=LOWER, u=UPPER, dtype=dtype)      # warm-up
        t0 = time.perf_counter()
        res, _ = M.optimizeLeastSquaresBatched(M.MODEL_EXP_DECAY_PAD8, x0b[:SAMPLE], t, data[:SAMPLE], l=LOWER, u=UPPER, dtype=dtype)
        per = (time.perf_counter() - t0) * 1e3 / SAMPLE
        lines += [f"  (d) host entry without the bit      {per:9.4f} ms a problem on the first {SAMPLE} (host clock; all statuses >= 0: "
                  f"{all(r.status >= 0 for r in res)}) -> {per * COUNT:.0f} ms for {COUNT} (extrapolated)",
                  f"  (a)/(c) {med['a'] / med['c']:.3f}   (b)/(c) {med['b'] / med['c']:.3f}   (d)/(a) {per * COUNT / med['a']:.0f}", ""]
    text = "\n".join(lines)
    print(text)
    if not args.only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
