"""Cost of the extra point of MIR_LSQ_FD_BASE_POINT at n = 128 (m = 1e6 by default): the caller-side difference-panel GEMM with
p = 2n against p = 2n + 1 (the extra residual vector formed from the stage of A in LDS), next to the one-point sweep the combined
call replaces, and the p = 2n call of other builds of the workload library (the parent's). HIP events over 20 launches per case,
five rounds with the cases interleaved: median (min .. max) per case; then the bits of the p = 2n + 1 output against the two
separate calls.
usage: gemm_base_point_ab.py [m] [paths of other builds of the workload library]"""
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
X = np.empty((p + 1, n)); X[:p] = np.tile(d["x0"], (p, 1)); X[ar, ar // 2] += 1e-8 * (1 - 2 * (ar % 2)); X[p] = d["x0"]
dX = api.DeviceBuffer(X)
dY = api.DeviceBuffer(nbytes=(m * n + m) * 8, dtype=np.float64, shape=(m * n + m,))
dy = api.DeviceBuffer(nbytes=m * 8, dtype=np.float64, shape=(m,))
WL = api.workloads_lib()
# RTLD_DEEPBIND: see gemm_only.py
others = [(path, C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)) for path in sys.argv[2:]]
ctx = C.c_void_p(C.addressof(prob.ctx))
sz = C.c_size_t


def panel(lib, entry, pts):
    return lambda: getattr(lib, entry)(ctx, sz(m), sz(n), sz(pts), C.c_void_p(dX.ptr), C.c_void_p(dY.ptr))


def point(lib):
    return lambda: lib.wl_tanh_linear_f_d(ctx, sz(m), sz(n), C.c_void_p(dX.ptr + p * n * 8), C.c_void_p(dy.ptr))


cases = [("forked, p = 2n", panel(WL, "wl_tanh_linear_fbd_d", p)), ("forked, p = 2n + 1", panel(WL, "wl_tanh_linear_fbd_d", p + 1)),
         ("dense, p = 2n", panel(WL, "wl_tanh_linear_fbd_dense_d", p)), ("dense, p = 2n + 1", panel(WL, "wl_tanh_linear_fbd_dense_d", p + 1)),
         ("one-point sweep", point(WL))]
for path, other in others:
    cases.append((f"other build {len(cases)}: forked, p = 2n", panel(other, "wl_tanh_linear_fbd_d", p)))
    cases.append((f"other build {len(cases) - 1}: one-point sweep", point(other)))
s = torch.cuda.ExternalStream(prob.stream.handle)
for _, fn in cases:
    for _ in range(3): fn()
prob.stream.synchronize()
times = {c[0]: [] for c in cases}
with torch.cuda.stream(s):
    for _ in range(5):
        for name, fn in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(20): fn()
            b.record(s)
            prob.stream.synchronize()
            times[name].append(a.elapsed_time(b) / 20)
print(f"m={m} n={n}: ms per call, median (min .. max) of 5 x 20 launches")
for name, t in times.items():
    t = sorted(t)
    print(f"  {name:56s} {t[2]:.4f} ({t[0]:.4f} .. {t[-1]:.4f})")
med = {k: sorted(v)[2] for k, v in times.items()}
print(f"  extra point inside the forked GEMM: {1e3 * (med['forked, p = 2n + 1'] - med['forked, p = 2n']):+.1f} us; "
      f"the sweep it replaces: {1e3 * med['one-point sweep']:.1f} us")
cases[0][1](); point(WL)(); prob.stream.synchronize()
D0, y0 = dY.download()[:m * n].copy(), dy.download().copy()
for name in ("forked, p = 2n + 1", "dense, p = 2n + 1"):
    dict(cases)[name](); prob.stream.synchronize()
    D = dY.download()
    same = np.array_equal(D[:m * n].view(np.uint64), D0.view(np.uint64)) and np.array_equal(D[m * n:].view(np.uint64), y0.view(np.uint64))
    print(f"  bits of '{name}' == panel of p = 2n + the one-point sweep: {same}")
    if not same:
        sys.exit(1)
