"""bench.py's command line: a plain run carries only the headline (the other legs need --full), and --dump-outputs writes
what the last timed step computed.
  CPU: option handling and the output writer
  GPU: a small plain cfg-3 run with --dump-outputs, outputs against the JSON line"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def parse(monkeypatch, *argv):
    # bench.py sets an environment default when it is imported: keep it inside this test
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_turns_the_other_legs_off(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.survey_steps == 0 and a.no_host_callback and a.no_cpu_baseline and a.cfg5_replicas == 1


def test_full_keeps_the_other_legs_and_their_options(monkeypatch):
    a = parse(monkeypatch, "--full")
    assert a.survey_steps == 10 and not a.no_host_callback and not a.no_cpu_baseline and a.cfg5_replicas == 16
    a = parse(monkeypatch, "--full", "--survey-steps", "1", "--no-cpu-baseline", "--dump-outputs", "out")
    assert a.survey_steps == 1 and a.no_cpu_baseline and not a.no_host_callback and a.dump_outputs == "out"


def test_dump_outputs_writes_float_arrays(tmp_path):
    from benchlib.common import dump_outputs
    dump_outputs(str(tmp_path / "d"), {"x": np.arange(3, dtype=np.float32), "status": [1], "n": np.array([2, 3])})
    x, st, n = (np.load(tmp_path / "d" / f"{k}.npy") for k in ("x", "status", "n"))
    assert x.dtype == np.float32 and st.dtype == np.float64 and n.dtype == np.float64
    assert x.tolist() == [0, 1, 2] and st.tolist() == [1] and n.tolist() == [2, 3]
    with pytest.raises(SystemExit):
        dump_outputs(str(tmp_path / "big"), {"a": np.zeros((64 << 20) // 8 + 1)})
    assert not (tmp_path / "big").exists()


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_step_computed(tmp_path):
    env = dict(os.environ, BENCH_M="200000", BENCH_N="64")
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith('{"metric"')][-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"] == "f64"
    assert d["value"] == pytest.approx(d["config"]["iterations_per_solve"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["config"]["survey_setting"] is None
    assert not {"cpu_baseline", "cpu_baseline_1thread", "host_callback_mode"} & set(d)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"x", "status", "iterations", "fcalls", "gcalls", "residual", "lambda"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["x"].shape == (64,) and np.isfinite(got["x"]).all()
    # every step is the same solve: the last one's result is the line's
    assert got["residual"][0] == d["config"]["residual"] and got["fcalls"][0] == d["config"]["fcalls_per_solve"]
    assert got["iterations"][0] == d["config"]["iterations_per_solve"]
