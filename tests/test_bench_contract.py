"""bench.py's output contract: exactly one JSON line on stdout whatever libraries print there, the headline line still
comes out when the multi-GPU extra never returns, and `--dump-outputs` writes what the last timed step computed."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = f"""
import importlib.util, os, sys, time
spec = importlib.util.spec_from_file_location("bench", {os.path.join(ROOT, "bench.py")!r})
bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
"""


def run(body: str):
    p = subprocess.run([sys.executable, "-c", PRELUDE + body], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


def test_stdout_is_reserved_for_the_line():
    rc, out, err = run("""
bench.reserve_stdout()
os.write(1, b"banner written by a C library\\n")   # what RCCL does at communicator creation
print("and a stray Python print")
bench.emit_line({"metric": "m", "value": 1.0})
""")
    assert rc == 0
    lines = out.splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == {"metric": "m", "value": 1.0}
    assert "banner written by a C library" in err and "stray Python print" in err


def test_deadline_prints_the_headline_and_leaves():
    rc, out, err = run("""
bench.reserve_stdout()
args = type("A", (), {"workload": "importance"})()
g = bench.ExtrasDeadline(0, {"metric": "m", "value": 2.0, "n_gpus": 2}, 0.2, "smc_lgssm_sharded", args)
time.sleep(30)          # a rank stuck in a collective
bench.emit_line({"never": "reached"})
""")
    assert rc == 3  # a hang is a failed run: the headline is printed, the status is non-zero
    lines = out.splitlines()
    assert len(lines) == 1
    o = json.loads(lines[0])
    assert o["value"] == 2.0 and "error" in o["extra"]["smc_lgssm_sharded"]
    assert "deadline" in err


def test_deadline_not_rank0_prints_nothing_and_finish_disarms():
    rc, out, err = run("""
g = bench.ExtrasDeadline(1, None, 0.2, "x")
time.sleep(30)
""")
    assert rc == 3 and out == ""
    rc, out, err = run("""
g = bench.ExtrasDeadline(0, {"value": 3.0}, 0.3, "x")
assert g.claim_line() and not g.claim_line()
bench.emit_line({"value": 3.0, "extra": {"x": 1}})
g.finish()
time.sleep(0.8)
print("alive", file=sys.stderr)
""")
    assert rc == 0 and "alive" in err
    assert [json.loads(l) for l in out.splitlines()] == [{"value": 3.0, "extra": {"x": 1}}]


def test_gpus_n_without_n_gpus_fails_loudly():
    """`python bench.py --gpus 2` on a box with fewer than 2 GPUs: exit status 2 and a message, never a line that says
    n_gpus 1 (the parent process counts devices without initialising the GPU runtime and starts nothing)."""
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has the GPUs: the command would run")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 2 and p.stdout.strip() == "" and "refusing" in p.stderr


def test_dump_outputs_stays_under_the_cap_with_a_seeded_sample(tmp_path):
    """Columns that would pass DUMP_MAX_BYTES are cut to the same seeded, sorted sample of particles in every file."""
    rc, out, err = run(f"""
import numpy as np, torch
n = 1_500_000
cols = {{"values": torch.arange(10 * n, dtype=torch.float32).reshape(10, n) % n, "logw": torch.arange(n, dtype=torch.float32)}}
for d in ("a", "b"):
    bench.dump_outputs(os.path.join({str(tmp_path)!r}, d), cols, {{"log_z": -1.25}})
""")
    assert rc == 0, err
    import numpy as np

    for d in ("a", "b"):
        p = tmp_path / d
        assert sum(f.stat().st_size for f in p.iterdir()) <= 64_000_000
        idx = np.load(p / "sample_index.npy")
        assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
        assert np.array_equal(np.load(p / "logw.npy"), idx.astype(np.float32))
        assert np.array_equal(np.load(p / "values.npy")[3], idx.astype(np.float32))
        assert np.load(p / "log_z.npy").tolist() == [-1.25]
    assert np.array_equal(np.load(tmp_path / "a" / "sample_index.npy"), np.load(tmp_path / "b" / "sample_index.npy"))


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path, oracle_ops):
    """A plain run: one line with the contract's fields, ONE timed block whose time is K x `ms_per_step`, nothing from
    `--full`; its dump holds the last timed step, equal bit for bit to the oracle's pass.  K = 35: 32 passes per launch and
    fold batch, so the last step is the third pass of the second batch's one launch (seed 2)."""
    import numpy as np
    import torch

    from genjax._amd import workloads as W

    n = 200_000
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "35", "--warmup", "1", "--particles", str(n),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 35 and d["timed_blocks"] == 1 and d["higher_is_better"] is True
    assert abs(d["block_ms_median"] / d["ms_per_step"] - 35) < 1e-9
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / n - 1.0) < 1e-9
    assert d["cpu_baseline"] is None and "extra" not in d
    o = W.gaussian10_importance(oracle_ops, impl=1, seed=2, n=n)
    assert np.array_equal(np.load(tmp_path / "logw.npy"), o["logw"].numpy())
    assert np.array_equal(np.load(tmp_path / "score.npy"), o["score"].numpy())
    assert np.array_equal(np.load(tmp_path / "values.npy"), torch.stack(list(o["values"])).numpy())
    assert np.load(tmp_path / "log_z.npy").tolist() == [o["log_z_rows"]]


@pytest.mark.gpu
def test_plain_smc_run_times_whole_runs_and_dumps_the_last_one(tmp_path, oracle_ops):
    """`--workload smc_lgssm`: a timed step is one whole T = 100 filter run; ONE block of K runs, `value` x `ms_per_step` the
    particle-steps of one run; the dump (every run is the same seeded filter) equals the oracle's filter bit for bit."""
    import numpy as np

    from genjax._amd import workloads as W

    n, T = 102_400, 100
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "smc_lgssm", "--steps", "3", "--warmup", "1",
                        "--particles", str(n), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["timed_blocks"] == 1 and abs(d["block_ms_median"] / d["ms_per_step"] - 3) < 1e-9
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / (n * T) - 1.0) < 1e-9
    assert d["cpu_baseline"] is None and "extra" not in d
    wl = W.LgssmSMC(oracle_ops, 1, 1, n, T)  # bench.py's workload (seed 1), on the oracle
    o = wl.result(wl.run())
    assert np.array_equal(np.load(tmp_path / "state.npy"), o["state"].numpy())
    assert np.array_equal(np.load(tmp_path / "logw.npy"), o["logw"].numpy())
    assert np.load(tmp_path / "log_z.npy").tolist() == [o["log_z"]]
