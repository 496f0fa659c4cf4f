"""What the bound stride of the batched kernels costs (MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM), measured on the GPU.

    python scripts/batched_problem_bounds.py measure OUT.json [TREE]
HIP events around ONE kernel-entry launch of 4096 problems at m = 512 (starts uploaded before, untimed; caller-owned basis
table), median of 25 launches after 2 warm-ups, as scripts/batched_f64.py and scripts/batched16.py measure, for
  * EXP_DECAY_PAD8 (n = 8) in f32 and f64, the default instance and MIR_LSQ_BATCHED_DEVICE_BOUNDS (mir_lsq_batched_kernel_ex_*),
  * EXP_HARM16 (n = 16, mir_lsq_batched16_kernel_ex_d),
  * the two covariance kernels alone on those fits' records (mir_lsq_batched_covariance_s / _d, mir_lsq_batched16_covariance_d),
each with SHARED bounds (n values, infinite: the launches every earlier measurement made) and -- where the library of TREE knows
the flag -- with the same box replicated count x n and the flag set: the same fits, so any difference is the cost of the stride.
TREE (default: this checkout) is the root of a built checkout whose mir_optim_amd package is measured: a checkout of the
parent commit gives the figures to compare with. The problem generators are this checkout's tests/batched16_problems.py.

    python scripts/batched_problem_bounds.py report PARENT_1.json PARENT_2.json BRANCH.json [directory]
writes profiles/r18/batched_problem_bounds.txt: per family the two parent runs, the branch, the per-problem launch, and the rule
of profiles/r15: the branch's median may exceed the slower parent run by no more than the two parent runs differ."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, MROWS, REPS = 4096, 512, 25
PER_PROBLEM, DEVICE_BOUNDS = 2, 4


def measure(out, tree):
    import torch
    sys.path.insert(0, os.path.abspath(tree))
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import mir_optim_amd as M
    from mir_optim_amd import api
    import batched16_problems as PR                                        # tests/: the problem generators
    assert os.path.abspath(M.__file__).startswith(os.path.abspath(tree)), (M.__file__, tree)
    torch.cuda.init()
    L = api.lib()
    knows_flag = hasattr(M, "BATCHED_BOUNDS_PER_PROBLEM")
    stream = torch.cuda.current_stream().cuda_stream

    def launcher(fn, model, dtype, nb, x0, t, data, variant, per_problem, recs=None, xfit=None):
        """(upload, run, download) of one launch; a covariance entry (recs given) runs on the records and x of a fit"""
        count, n = x0.shape
        item = np.dtype(dtype).itemsize
        s = M.LeastSquaresSettings(dtype)
        shape = (count, n) if per_problem else (n,)
        arrays = (t, data, x0 if xfit is None else xfit, np.full(shape, -np.inf), np.full(shape, np.inf))
        b = [api.DeviceBuffer(np.ascontiguousarray(a, dtype=dtype)) for a in arrays]
        rsize = 24 if dtype == np.float32 else 32
        res = api.DeviceBuffer(nbytes=count * rsize, dtype=np.uint8, shape=(count * rsize,)) if recs is None else api.DeviceBuffer(recs)
        basis = api.DeviceBuffer(nbytes=MROWS * nb * item, dtype=dtype, shape=(MROWS, nb))
        cov = api.DeviceBuffer(nbytes=count * n * n * item, dtype=dtype, shape=(count, n, n)) if recs is not None else None
        opt = api.BatchedOptions(stream=stream, basis=basis.ptr, basis_bytes=basis.nbytes, variant=variant)
        ex = api.BatchedExtras(flags=PER_PROBLEM if per_problem else 0, covariance=cov.ptr if cov else None)
        x0c = np.ascontiguousarray(x0, dtype=dtype)

        def upload():
            if recs is None:
                assert L.mir_lsq_memcpy_h2d(b[2].ptr, x0c.ctypes.data, x0c.nbytes, C.c_void_p(stream)) == 0

        def run():
            rc = fn(C.byref(s), count, MROWS, model, b[2].ptr, b[3].ptr, b[4].ptr, b[0].ptr, 0, b[1].ptr, res.ptr, C.byref(opt), C.byref(ex))
            assert rc == 0, rc

        def download():
            torch.cuda.synchronize()
            return res.download().copy(), b[2].download().copy(), (cov.download().copy() if cov else None)
        run.keep = (b, res, basis, cov, opt, ex, s, x0c)
        return upload, run, download

    def timed(upload, run):
        for _ in range(2):
            upload(); run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            upload()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))]

    t8, d8, x8 = PR.pad8_problems(COUNT, MROWS)
    t16, _, d16, _, x16 = PR.harm_problems(16, MROWS, COUNT)
    fits = [("PAD8 f32 default", L.mir_lsq_batched_kernel_ex_s, L.mir_lsq_batched_covariance_s, M.MODEL_EXP_DECAY_PAD8, np.float32, 4, x8, t8, d8, 0),
            ("PAD8 f32 DEVICE_BOUNDS", L.mir_lsq_batched_kernel_ex_s, None, M.MODEL_EXP_DECAY_PAD8, np.float32, 4, x8, t8, d8, DEVICE_BOUNDS),
            ("PAD8 f64 default", L.mir_lsq_batched_kernel_ex_d, L.mir_lsq_batched_covariance_d, M.MODEL_EXP_DECAY_PAD8, np.float64, 4, x8, t8, d8, 0),
            ("PAD8 f64 DEVICE_BOUNDS", L.mir_lsq_batched_kernel_ex_d, None, M.MODEL_EXP_DECAY_PAD8, np.float64, 4, x8, t8, d8, DEVICE_BOUNDS),
            ("EXP_HARM16 f64", L.mir_lsq_batched16_kernel_ex_d, L.mir_lsq_batched16_covariance_d, M.MODEL16_EXP_HARM16, np.float64, 13, x16, t16, d16, 0)]
    figures = {}
    for label, fit, covfn, model, dtype, nb, x0, t, data, variant in fits:
        shared = launcher(fit, model, dtype, nb, x0, t, data, variant, False)
        figures[label] = {"shared": timed(shared[0], shared[1])}
        recs, xfit, _ = shared[2]()
        if knows_flag:
            own = launcher(fit, model, dtype, nb, x0, t, data, variant, True)
            figures[label]["per_problem"] = timed(own[0], own[1])
            r2, x2, _ = own[2]()
            assert r2.tobytes() == recs.tobytes() and x2.tobytes() == xfit.tobytes(), label          # the same fits, bit for bit
        if covfn is not None:
            clabel = label.replace(" default", "") + " covariance alone"
            cs = launcher(covfn, model, dtype, nb, x0, t, data, variant, False, recs=recs, xfit=xfit)
            figures[clabel] = {"shared": timed(cs[0], cs[1])}
            c1 = cs[2]()[2]
            assert np.isfinite(c1).all(), clabel
            if knows_flag:
                co = launcher(covfn, model, dtype, nb, x0, t, data, variant, True, recs=recs, xfit=xfit)
                figures[clabel]["per_problem"] = timed(co[0], co[1])
                assert co[2]()[2].tobytes() == c1.tobytes(), clabel
        print(label, figures[label], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump({"tree": os.path.abspath(tree), "knows_flag": knows_flag, "count": COUNT, "m": MROWS, "reps": REPS, "figures": figures},
              open(out, "w"), indent=1)


def report(p1, p2, br, out):
    a, b, c = (json.load(open(p)) for p in (p1, p2, br))
    assert not a["knows_flag"] and not b["knows_flag"] and c["knows_flag"], "two runs of the parent, then the branch"
    lines = [f"the bound stride of the batched kernels (MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM): {c['count']} problems, m = {c['m']}; HIP events "
             f"around ONE kernel-entry launch (starts uploaded before, untimed), median of {c['reps']} launches after 2 warm-ups, ms.",
             "shared bounds at the parent commit (two separate runs) and at the branch; rule (profiles/r15): the branch may exceed the",
             "slower parent run by no more than the two parent runs differ. per-problem: the same batch with the box replicated count x n",
             "(the same fits, bit for bit): its difference to the branch's shared launch is the cost of the stride.",
             "",
             f"  {'family':34s} {'parent 1':>9s} {'parent 2':>9s} {'spread':>8s} {'branch':>9s} {'over slower':>12s}  rule   {'per-problem':>11s} {'ratio':>7s}"]
    missed = []
    for label, fig in c["figures"].items():
        x1, x2, y = a["figures"][label]["shared"][0], b["figures"][label]["shared"][0], fig["shared"][0]
        spread, over = abs(x1 - x2), y - max(x1, x2)
        ok = over <= spread
        if not ok:
            missed.append(label)
        pp = fig["per_problem"][0]
        lines.append(f"  {label:34s} {x1:9.4f} {x2:9.4f} {spread:8.4f} {y:9.4f} {over:+12.4f}  {'ok  ' if ok else 'MISS'}   {pp:11.4f} {pp / y:7.4f}")
    lines += ["", "families that missed the rule: " + (", ".join(missed) if missed else "none")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(out, exist_ok=True)
    open(os.path.join(out, "batched_problem_bounds.txt"), "w").write(text)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "measure":
        measure(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else ROOT)
    elif len(sys.argv) >= 5 and sys.argv[1] == "report":
        report(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "r18"))
    else:
        sys.exit(__doc__)
