"""N > 1 path: rows sharded over ranks, sum all-reduce of [J^T J | J^T y] and of the residual
scalars, everything else replicated. world_size 2 over gloo on 127.0.0.1.
  CPU  : host logic (row_shard, payload length) + the oracle's sharded restatement == the unsharded oracle
  GPU  : the HIP path with the callback communicator, two processes sharing the GPU == the unsharded oracle"""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import problems as P
from mir_optim_amd import parallel as PAR

HERE = os.path.dirname(os.path.abspath(__file__))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(mode, m_total, n, tmp_path, world=2):
    out = str(tmp_path / "result")
    port = str(free_port())
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   LOCAL_RANK=str(r), OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker.py"), mode, str(m_total), str(n), out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return [json.load(open(f"{out}.{r}")) for r in range(world)]


def unsharded_oracle(oracle, m_total, n):
    w = P.tanh_linear(m_total, n)
    s = oracle.default_settings(); s.absTolerance = 1e-9
    ctx = oracle.TanhLinearCtx(w["A"].ctypes.data, w["b"].ctypes.data)
    return oracle.optimize(oracle.native_fn("wlc_tanh_linear_f"), m_total, w["x0"], settings=s, fctx=C.addressof(ctx))


def test_row_shard_partition():
    for m_total, world in [(10, 2), (11, 2), (1000000, 8), (7, 8), (8000000, 8), (5, 3)]:
        blocks = [PAR.row_shard(m_total, world, r) for r in range(world)]
        assert blocks[0][0] == 0 and sum(b[1] for b in blocks) == m_total
        for (o0, l0), (o1, _) in zip(blocks, blocks[1:]):
            assert o0 + l0 == o1                                  # contiguous, no gap / overlap
        assert max(b[1] for b in blocks) - min(b[1] for b in blocks) <= 1
    assert PAR.packed_length(128) == 8384 and PAR.packed_length(256) == 33152   # 66 KB / 259 KB payloads
    # shards concatenate to the unsharded data set (bit-identical inputs across world sizes)
    full = P.tanh_linear(1001, 8)
    parts = [P.tanh_linear(l, 8, row_offset=o) for o, l in (PAR.row_shard(1001, 3, r) for r in range(3))]
    assert np.array_equal(np.vstack([p["A"] for p in parts]), full["A"])
    assert np.array_equal(np.concatenate([p["b"] for p in parts]), full["b"])


def test_sharded_oracle_matches_unsharded_gloo(oracle, tmp_path):
    m_total, n = 6001, 12
    res = launch("oracle", m_total, n, tmp_path)
    ro, xo = unsharded_oracle(oracle, m_total, n)
    assert res[0]["x"] == res[1]["x"] and res[0]["iterations"] == res[1]["iterations"]    # replicas agree bit for bit
    assert np.allclose(res[0]["x"], xo, rtol=1e-7, atol=1e-10)
    assert np.isclose(res[0]["residual"], ro.residual, rtol=1e-10)
    assert (res[0]["status"] not in ("maxIterations", "numericError")) and ro.status >= 0


@pytest.mark.gpu
def test_sharded_gpu_path_matches_unsharded_oracle(oracle, tmp_path):
    m_total, n = 40000, 64
    res = launch("gpu", m_total, n, tmp_path)
    ro, xo = unsharded_oracle(oracle, m_total, n)
    assert res[0]["x"] == res[1]["x"] and res[0]["iterations"] == res[1]["iterations"]    # replicas agree bit for bit
    assert np.allclose(res[0]["x"], xo, rtol=1e-6, atol=1e-9)
    assert np.isclose(res[0]["residual"], ro.residual, rtol=1e-9)
    assert res[0]["status"] not in ("maxIterations", "numericError")


@pytest.mark.gpu
def test_rccl_communicator_world_size_1(oracle):
    """The production communicator (RCCL via dlopen) on the one visible GPU: id creation, ncclCommInitRank,
    fp64 sum all-reduce of the packed buffer and of the residual scalar on the solver's stream, destroy."""
    import mir_optim_amd as M
    from mir_optim_amd import workloads as W
    comm = PAR.rccl_comm(1, 0, lambda buf: buf)
    assert M.api.lib().mir_lsq_comm_ranks(comm) == 1                  # ncclCommCount
    assert PAR.check_comm(comm, 1, 0)                                 # mir_lsq_comm_allreduce_d: the bench's self-check
    for n in (32, 128):
        w = P.tanh_linear(30000, n)
        prob = W.TanhLinear(w["A"], w["b"])
        s = M.LeastSquaresSettings(); s.absTolerance = 1e-9
        st = M.Stats()
        r1, x1 = prob.solve(w["x0"], settings=s, comm=comm, stats=st, batched=True)
        r0, x0 = prob.solve(w["x0"], settings=s, batched=True)
        assert r1.status >= 0 and np.array_equal(x1, x0) and r1.iterations == r0.iterations   # sum over one rank = identity
        # every exchange of the solve went through ncclAllReduce with the documented payloads (n = 128: 8384 / 291 / 1+)
        assert st.allreduce_calls[0] == st.jacobian_full + st.jtj_resyncs >= 1
        assert st.allreduce_elems[0] == st.allreduce_calls[0] * PAR.packed_length(n)
        # COLLECTIVE BUDGET (the three reductions LS:1052, 1065, 1115): a fused round exchanges [sweep | trial sum] ONCE; only a
        # Broyden pass that no fused round had prepared pays a sweep exchange of its own, only a trial that did not ride on a
        # sweep (and the entry residual) a scalar one
        assert st.fused_rounds >= st.fused_passes >= 1 and st.jacobian_broyden >= st.fused_passes
        assert st.allreduce_calls[1] == st.fused_rounds + (st.jacobian_broyden - st.fused_passes)
        assert st.allreduce_elems[1] == st.allreduce_calls[1] * (2 * n + 35)
        assert st.allreduce_calls[2] == 1 + (st.trial_callback_calls - st.fused_rounds) and st.allreduce_elems[2] >= st.allreduce_calls[2]
    # cfg 3's own trajectory at the bench's tolerance (refresh, 4 Broyden passes, confirming refresh; 6 trials): 1 + 2 + 6 = 9
    # exchanges per solve (13 with one-by-one rounds)
    w = P.tanh_linear(30000, 128)
    prob = W.TanhLinear(w["A"], w["b"])
    s = M.LeastSquaresSettings(); s.absTolerance = 1e-5
    counts = {}
    for variant in (0, M.VARIANT_NO_PIPELINE):
        st = M.Stats()
        r1, x1 = prob.solve(w["x0"], settings=s, comm=comm, stats=st, batched=True, variant=variant)
        counts[variant] = (sum(st.allreduce_calls), st.trial_callback_calls, st.jacobian_full, st.jacobian_broyden, x1.tobytes(), r1.residual)
        if not variant:
            assert st.fused_passes == st.jacobian_broyden            # every Broyden pass of this trajectory rode on a fused round
    assert counts[0][1:] == counts[M.VARIANT_NO_PIPELINE][1:]
    trials, full, broyden = counts[0][1:4]
    assert (counts[0][0], counts[M.VARIANT_NO_PIPELINE][0]) == (1 + full + trials, 1 + full + broyden + trials), (counts[0][:4], counts[M.VARIANT_NO_PIPELINE][:4])
    assert PAR.packed_length(128) == 8384 and 2 * 128 + 35 == 291
    M.api.lib().mir_lsq_comm_destroy(comm)


@pytest.mark.gpu
def test_bench_two_ranks_rehearsal_on_one_gpu():
    """bench.py through torch.distributed.run with two ranks sharing the GPU (callback communicator over gloo): rank 0
    prints one JSON line, last; both shards contribute; the control flow of the N > 1 path (barriers, max over ranks,
    teardown) completes."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, BENCH_M="200000", BENCH_N="64", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--comm", "gloo-callback", "--full", "--survey-steps", "1"]
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    d = json.loads(lines[-1])
    assert sum(1 for l in lines if l.startswith('{"metric"')) == 1
    # default = strong scaling: the SAME 200000-row problem split over the two ranks; value = the global solve's it/s
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "strong"
    assert d["config"]["m_total"] == 200000 and d["config"]["m_per_gpu"] == 100000
    assert d["config"]["status"] in ("xConverged", "furtherImprovement", "fConverged", "gConverged")
    assert d["value"] == pytest.approx(d["config"]["iterations_per_solve"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["config"]["survey_setting"]["abs_tolerance"] == 1e-9 and d["config"]["survey_setting"]["value"] > 0
    assert d["config"]["allreduce_per_solve"]["packed_elems"] == 64 * 65 // 2 + 64
    assert d["value"] > 0 and d["roofline"]["frac"] > 0 and "cpu_baseline" not in d


@pytest.mark.gpu
def test_bench_falls_back_when_rccl_is_unusable():
    """bench.py --comm rccl with two ranks on ONE GPU: RCCL refuses two ranks on the same device (ncclCommInitRank fails on
    both), every rank takes the same decision over the control plane and the run continues on the callback communicator --
    one JSON line that says so, instead of a crash or a hang in the driver's multi-GPU run."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, BENCH_M="100000", BENCH_N="32", OMP_NUM_THREADS="2",
               BENCH_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--survey-steps", "0", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith('{"metric"')][-1])
    assert d["n_gpus"] == 2 and d["config"]["rccl_fallback_reason"] and "callback" in d["config"]["parallelism"]
    assert d["config"]["status"] in ("xConverged", "furtherImprovement", "fConverged", "gConverged") and d["value"] > 0


def test_bench_self_launch_reports_a_failed_rank_and_prints_no_line():
    """`python bench.py --gpus 2` from a bare shell starts its own rank processes (bench.py: launch_ranks). With no usable
    GPU every rank exits non-zero: the parent must exit non-zero too, print no JSON line and leave no rank behind."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--comm", "gloo-callback"], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode != 0
    assert p.stdout.decode().strip() == ""
    assert "stopping the other ranks" in p.stderr.decode()


@pytest.mark.gpu
def test_bench_self_launches_its_ranks_from_a_bare_shell():
    """The driver's command, literally: `python3 bench.py --gpus 2 --steps 3 --warmup 1` with no launcher around it. The
    parent starts two rank processes (sharing the one GPU here: BENCH_SHARE_GPU=1, callback communicator over gloo) and
    relays rank 0's line as its own LAST stdout line."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, BENCH_M="200000", BENCH_N="64", OMP_NUM_THREADS="2", BENCH_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--comm", "gloo-callback"]
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"')          # the parent's stdout is the line and nothing else
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "strong"
    assert d["config"]["m_total"] == 200000 and d["config"]["m_per_gpu"] == 100000
    assert d["config"]["launcher"].startswith("bench.py") and d["config"]["ranks_share_gpus"] is True
    assert d["config"]["status"] in ("xConverged", "furtherImprovement", "fConverged", "gConverged")
    assert d["value"] == pytest.approx(d["config"]["iterations_per_solve"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["config"]["allreduce_per_solve"]["packed_elems"] == 64 * 65 // 2 + 64
    assert d["value"] > 0 and d["roofline"]["frac"] > 0 and "cpu_baseline" not in d


@pytest.mark.gpu
def test_bench_self_launch_with_rccl_on_one_gpu_takes_the_labelled_fallback():
    """`python3 bench.py --gpus 2` (default --comm rccl) on a box with ONE GPU and nothing in the environment: the ranks share
    the device, RCCL refuses the communicator, every rank switches to the callback communicator -- a labelled line, rc 0."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, BENCH_M="100000", BENCH_N="32", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BENCH_SHARE_GPU"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--survey-steps", "0"]
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["config"]["rccl_fallback_reason"] and "callback" in d["config"]["parallelism"]
    assert d["config"]["ranks_share_gpus"] is True and d["config"]["visible_gpus"] == 1
    assert d["config"]["status"] in ("xConverged", "furtherImprovement", "fConverged", "gConverged") and d["value"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("extra,m_env,check", [
    ([], "80000", lambda d: d["scaling"] == "strong" and d["config"]["m_total"] == 80000),
    (["--scaling", "weak", "--n", "256"], "12000", lambda d: d["scaling"] == "weak" and d["config"]["m_per_gpu"] == 12000
     and d["config"]["m_total"] == 4 * 12000 and d["config"]["allreduce_per_solve"]["packed_elems"] == 256 * 257 // 2 + 256),
])
def test_bench_four_rank_rehearsal_on_one_gpu(extra, m_env, check):
    """First-contact rehearsal for the driver's multi-GPU run: `python bench.py --gpus 4` from a bare shell with FOUR rank
    processes sharing the one GPU (the box admits at most six processes on its card and this test process is one of them --
    six ranks got the run killed by the box's process guard; the driver's N = 8 is four more of the same). Port, rendezvous, deadline, barriers, max over ranks and the JSON relay with more than two ranks -- strong scaling
    (the headline's command line) and `--scaling weak --n 256` (cfg 4's), so that neither flag pair meets the launcher for the
    first time on the 8-GPU node."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, BENCH_M=m_env, OMP_NUM_THREADS="2", BENCH_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BENCH_N"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1", "--comm", "gloo-callback",
           "--survey-steps", "0"] + extra
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"')
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["steps"] == 2 and d["config"]["ranks_share_gpus"] is True and check(d), d
    assert d["config"]["status"] in ("xConverged", "furtherImprovement", "fConverged", "gConverged") and d["value"] > 0
    assert d["value"] == pytest.approx(d["config"]["iterations_per_solve"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
