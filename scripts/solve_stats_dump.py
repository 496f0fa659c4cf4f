"""The bench problem (cfg 3: m = 1e6, n = 128, absTolerance 1e-5, batched FD) solved twice on one workspace with a Stats block, in the
tree of the CURRENT DIRECTORY (run it from the root of each tree of an A/B): every integer counter of the second solve, the result's
counters and the residual's bits as one JSON line (profiles/r27, r28: dump_outputs_compare.txt).

    python scripts/solve_stats_dump.py [VARIANT]      VARIANT: mir_lsq_gpu_options.variant, e.g. 4194304 = MIR_LSQ_VARIANT_NO_PIPELINE"""
import ctypes as C, json, os, sys
sys.path.insert(0, os.getcwd())
import mir_optim_amd as M
from mir_optim_amd import api, workloads as W
m, n = 1_000_000, 128
data = W.tanh_linear_data(m, n, row_offset=0)
prob = W.TanhLinear(data["A"], data["b"])
s = M.LeastSquaresSettings(); s.absTolerance = 1e-5
variant = int(sys.argv[1], 0) if len(sys.argv) > 1 else 0
ws = api.lib().mir_lsq_workspace_create(m, n, 8)
out = None
for _ in range(2):
    st = api.Stats()
    r, x = prob.solve(data["x0"], settings=s, stats=st, flags=0, workspace=ws, variant=variant, batched=True)
    out = {k: int(getattr(st, k)) for k, t in api.Stats._fields_ if t in (C.c_uint64, C.c_uint32, C.c_int32, C.c_int64)}
    out.update(status=r.status.name, iterations=int(r.iterations), fcalls=int(r.fCalls), gcalls=int(r.gCalls), residual=float(r.residual).hex())
print(json.dumps(out, sort_keys=True))
