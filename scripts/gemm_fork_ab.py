"""The caller-side difference-panel GEMM at n = 128 (m = 1e6 by default), default entry (prefix forking when X passes the check)
against the dense entry: on finite-difference X, and on X one ulp off in point 255, which fails the check (the default entry then
runs the dense GEMM behind the check: the check's cost). With the paths of other builds of the workload library (the parent's,
or variants of the group table), the default entry of each too. HIP events over 20 launches per case, five rounds with the cases
interleaved: median (min .. max) per case; then the bits of every panel against the dense entry's on the same X.
usage: gemm_fork_ab.py [m] [paths of other builds of the workload library]"""
import ctypes as C, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from mir_optim_amd import api, workloads as W
m = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
n, p = 128, 256
d = W.tanh_linear_data(m, n)
prob = W.TanhLinear(d["A"], d["b"])
ar = np.arange(p)
X = np.tile(d["x0"], (p, 1)); X[ar, ar // 2] += 1e-8 * (1 - 2 * (ar % 2))
Xbad = X.copy(); Xbad[255, 0] = np.nextafter(Xbad[255, 0], np.inf)
dX, dXb = api.DeviceBuffer(X), api.DeviceBuffer(Xbad)
dY = api.DeviceBuffer(nbytes=m * n * 8, dtype=np.float64, shape=(m, n))
WL = api.workloads_lib()
# RTLD_DEEPBIND: see gemm_only.py
others = [(path, C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)) for path in sys.argv[2:]]
cases = [("default entry, FD X (forked)", WL.wl_tanh_linear_fbd_d, dX, "dense, FD X"),
         ("dense entry, FD X", WL.wl_tanh_linear_fbd_dense_d, dX, None),
         ("default entry, X fails the check", WL.wl_tanh_linear_fbd_d, dXb, "dense, bad X"),
         ("dense entry, same X", WL.wl_tanh_linear_fbd_dense_d, dXb, None)]
for path, other in others:
    cases.append((f"{os.path.basename(path)} (other build), FD X", other.wl_tanh_linear_fbd_d, dX, "dense, FD X"))
ctx = C.c_void_p(C.addressof(prob.ctx))
s = torch.cuda.ExternalStream(prob.stream.handle)


def call(fn, x):
    fn(ctx, C.c_size_t(m), C.c_size_t(n), C.c_size_t(p), C.c_void_p(x.ptr), C.c_void_p(dY.ptr))


for _, fn, x, _r in cases:
    for _ in range(3): call(fn, x)
prob.stream.synchronize()
times = {c[0]: [] for c in cases}
with torch.cuda.stream(s):
    for _ in range(5):
        for name, fn, x, _r in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(20): call(fn, x)
            b.record(s)
            prob.stream.synchronize()
            times[name].append(a.elapsed_time(b) / 20)
print(f"m={m} n={n} p={p}: ms per call, median (min .. max) of 5 x 20 launches")
for name, t in times.items():
    t = sorted(t)
    print(f"  {name:48s} {t[2]:.4f} ({t[0]:.4f} .. {t[-1]:.4f})  {2.0 * m * n * p / t[2] / 1e9:.1f} TF dense-equivalent")
ref = {}
for name, fn, x, r in cases:
    call(fn, x)
    prob.stream.synchronize()
    D = dY.download()
    if r is None:
        ref["dense, FD X" if x is dX else "dense, bad X"] = D
for name, fn, x, r in cases:
    if r is None:
        continue
    call(fn, x)
    prob.stream.synchronize()
    D = dY.download()
    same = np.array_equal(D.view(np.uint64), ref[r].view(np.uint64))
    print(f"  bits of '{name}' == {r}: {same}")
    if not same:
        sys.exit(1)
