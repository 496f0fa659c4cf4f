#!/usr/bin/env python
"""What fitSpline on device-resident points costs (profiles/r19/fit_spline_gpu.txt).

  fit     np = 1e6 points, nx = 128 knots, f64, lambda = 1e-3 and 0: one warm-up, then the median wall time of `--reps` calls of
          mir_fit_spline_gpu_d with MIR_LSQ_TIME_KERNELS (points resident, a reused workspace is NOT passed: the entry's
          default). Per finite-difference refresh: fd_callback_ms / fd_callback_calls (table kernel + difference-panel kernel)
          next to the time the panel's m nx 8 bytes take at the measured plain-store HBM rate (6.0 TB/s), and the same callback
          at np = nx points, where the sweep is empty and the table kernel is what is left.
  parent  the same problem at np = 1e5 once through mir_fit_spline_d (host callbacks: the only way before this entry) and
          through mir_fit_spline_gpu_d (upload of the points included): wall time each, the ratio, and the largest difference
          of the fitted values.

Needs an MI355X.  python scripts/fit_spline_gpu_bench.py {fit,parent} [--reps 5] [--out FILE]  (the output is appended)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_STORE_TBS = 6.0     # plain 256-B wave stores, measured chip-wide


def problem(npoints, nx, seed=19):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.uniform(0.3, 2.0, nx))
    t = rng.uniform(x[0] - 0.5, x[-1] + 0.5, npoints)
    y = 3.0 * np.sin(0.7 * t) + 0.1 * t + rng.normal(0.0, 0.1, npoints)
    return x, np.column_stack([t, y])


def say(out, line):
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def run_fit(M, out, reps):
    nx, npoints = 128, 1000000
    x, pts = problem(npoints, nx)
    dev = M.DeviceBuffer(pts)
    lo, up = np.full(nx, -np.inf), np.full(nx, np.inf)
    say(out, f"# fit: np = {npoints}, nx = {nx}, f64, points resident; wall time of mir_fit_spline_gpu_d, median of {reps} after one warm-up")
    for lam in (1e-3, 0.0):
        walls, st = [], None
        for rep in range(reps + 1):
            st = M.Stats()
            t0 = time.perf_counter()
            r = M.fitSplineGpu(None, dev, x, lo, up, lam, stats=st)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                walls.append(wall)
        lr = r.leastSquaresResult
        m = npoints + (1 if lam == 0 else 0)
        per = st.fd_callback_ms / max(st.fd_callback_calls, 1)
        bound = m * nx * 8 / (HBM_STORE_TBS * 1e12) * 1e3
        say(out, f"lambda = {lam:g}: wall median {statistics.median(walls):.1f} ms (min {min(walls):.1f}, max {max(walls):.1f}); status {lr.status.name}, "
                 f"iterations {lr.iterations}, fCalls {lr.fCalls}, residual {lr.residual:.9g}")
        say(out, f"    refreshes {st.jacobian_full}, Broyden passes {st.jacobian_broyden}; fd callback {per:.3f} ms per call ({st.fd_callback_calls} calls, "
                 f"{st.fd_callback_points} points); panel write bound {bound:.3f} ms at {HBM_STORE_TBS} TB/s -> {per / bound:.2f} x the bound")
        say(out, f"    jtj_fd {st.jtj_fd_ms / max(st.jtj_fd_launches, 1):.3f} ms per launch ({st.jtj_fd_launches}); trial callbacks {st.trial_callback_ms:.2f} ms in "
                 f"{st.trial_callback_calls} calls; jtj {st.jtj_ms:.1f} ms, solve {st.solve_ms:.1f} ms, total {st.total_ms:.1f} ms")
    dev.free()
    # the table kernel's share: the same callback with an (almost) empty sweep
    xs, ps = problem(nx, nx)
    st = M.Stats()
    for _ in range(2):
        st = M.Stats()
        try:
            M.fitSplineGpu(None, ps, xs, lo, up, 1e-3, stats=st)
        except M.LeastSquaresException:      # as many points as knots: the fit may wander to maxIterations; the timings stand
            pass
    say(out, f"table kernel (+ a sweep over {nx} rows): fd callback {st.fd_callback_ms / max(st.fd_callback_calls, 1):.4f} ms per call at np = {nx} "
             f"({st.fd_callback_calls} calls)")


def run_parent(M, out):
    nx, npoints, lam = 128, 100000, 1e-3
    x, pts = problem(npoints, nx)
    lo, up = np.full(nx, -np.inf), np.full(nx, np.inf)
    M.fitSplineGpu(None, pts[:1000], x, lo, up, lam)             # warm-up of the runtime, not of the problem
    t0 = time.perf_counter()
    g = M.fitSplineGpu(None, pts, x, lo, up, lam)
    tg = time.perf_counter() - t0
    t0 = time.perf_counter()
    h = M.fitSpline(None, pts, x, lo, up, lam)
    th = time.perf_counter() - t0
    rg, rh = g.leastSquaresResult, h.leastSquaresResult
    say(out, f"# against the host-callback entry: np = {npoints}, nx = {nx}, f64, lambda = {lam:g}, one call each")
    say(out, f"mir_fit_spline_d     {th * 1e3:10.1f} ms  status {rh.status.name}, iterations {rh.iterations}, residual {rh.residual:.12g}")
    say(out, f"mir_fit_spline_gpu_d {tg * 1e3:10.1f} ms  status {rg.status.name}, iterations {rg.iterations}, residual {rg.residual:.12g}  (upload included)")
    say(out, f"ratio {th / tg:.1f} x; max |value difference| {np.abs(g.spline.values - h.spline.values).max():.3g}")
    if not tg < th:
        say(out, "CONDITION MISSED: the new entry is not faster")
        return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["fit", "parent"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "fit_spline_gpu.txt"))
    a = ap.parse_args()
    import mir_optim_amd as M
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.what == "fit":
        run_fit(M, a.out, a.reps)
        return 0
    return run_parent(M, a.out)


if __name__ == "__main__":
    sys.exit(main())
