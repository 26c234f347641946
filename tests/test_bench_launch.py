"""`bench.py --gpus N` as the driver may call it WITHOUT a launcher: the script starts its own ranks through
torch.distributed.run and rank 0 prints one JSON line.  Here (no GPU) the ranks only form the process group on gloo and
all-reduce one number (--rendezvous-only); the same launcher code starts the RCCL ranks on a GPU node."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_self_launches_its_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--dist-backend", "gloo",
                        "--rendezvous-only"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # only rank 0 prints
    out = json.loads(lines[0])
    assert out == {"rendezvous": "ok", "world": 2, "backend": "gloo", "allreduce_sum": 3.0}


def test_a_failing_child_rank_fails_the_bench():
    """rank 1 exits non-zero after the collective: the self-launching parent must pass a non-zero status on (the driver reads
    it), and a rank other than 0 never prints a result line"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--rendezvous-only",
                        "--rendezvous-fail-rank", "1"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0, r.stdout[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) <= 1 and all(json.loads(ln).get("rendezvous") == "ok" for ln in lines), r.stdout  # rank 0's line at most
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--rendezvous-only",
                        "--rendezvous-fail-rank", "0"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0 and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")], r.stdout  # rank 1 prints nothing


def test_bench_rejects_a_world_that_does_not_match():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rendezvous-only"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_workload_labels_name_the_right_baseline_config():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.workload_label("f32", 256, 16, False, 0, True).startswith("BASELINE configs[1]")
    assert bench.workload_label("bf16", 256, 32, False, 0, True).startswith("BASELINE configs[2]")
    assert bench.workload_label("bf16", 512, 8, False, 100, True).startswith("BASELINE configs[3]")
    assert "nudge every 100" in bench.workload_label("bf16", 512, 8, False, 100, True)
    assert bench.workload_label("bf16", 1024, 2, True, 0, True).startswith("BASELINE configs[4]")
    assert bench.workload_label("f32", 512, 8, False, 0, True).startswith("off-baseline")


def test_dump_sample_is_seeded_and_bounded(tmp_path):
    """--dump-outputs: small outputs are written whole in their shape, large ones as the same seeded sample every run"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    a = bench._dump_sample(small, 12, 1)
    assert a.dtype == np.float32 and a.shape == (3, 4) and (a == small.numpy()).all()
    big = torch.randn(10000)
    s1, s2, s3 = bench._dump_sample(big, 100, 7), bench._dump_sample(big, 100, 7), bench._dump_sample(big, 100, 8)
    assert s1.shape == (100,) and (s1 == s2).all() and not (s1 == s3).all()
    assert np.isin(s1, big.numpy()).all() and len(np.unique(s1)) == 100
    info = bench.write_outputs({"loss": np.zeros(3, np.float32), "params": s1}, str(tmp_path / "d"))
    assert info["files"] == ["loss.npy", "params.npy"] and info["bytes"] == 412
    assert (np.load(tmp_path / "d" / "params.npy") == s1).all()
    assert sum(bench.DUMP_CAP.values()) * 4 <= bench.DUMP_MAX_BYTES


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_every_run(cuda, tmp_path):
    """two runs with the same arguments: the same files, bit for bit, and ms_per_step / steps as asked"""
    import numpy as np
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--res", "64", "--batch", "2",
                            "--no-cpu-baseline", "--no-profile", "--no-extra-legs", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 3 and len(line["step_ms"]) == 3 and line["ms_per_step"] > 0
        files = sorted(os.listdir(d))
        assert files == line["dump_outputs"]["files"]
        assert {"loss.npy", "grad_norm.npy", "reconstruction.npy", "moments.npy", "latents.npy", "params.npy", "grads.npy"} <= set(files)
        dumps.append({f: np.load(d / f) for f in files})
    assert dumps[0].keys() == dumps[1].keys()
    for f, a in dumps[0].items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
        assert np.array_equal(a, dumps[1][f]), f
    assert dumps[0]["reconstruction.npy"].shape == (2, 3, 64, 64)
    assert np.allclose(dumps[0]["loss.npy"][2], dumps[0]["loss.npy"][0] + 1e-6 * dumps[0]["loss.npy"][1], rtol=1e-5)


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_legs(cuda):
    """a plain run times the steps and prints the headline only; --full adds the profiled region and the tracker A/B (the
    bf16 configs[2] leg only runs at the metric's shape, the CPU baseline is skipped here for time)"""
    common = ["--steps", "3", "--warmup", "1", "--res", "64", "--batch", "2"]
    lines = {}
    for mode in ([], ["--full", "--no-cpu-baseline"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + mode, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[bool(mode)] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    plain, full = lines[False], lines[True]
    for line in (plain, full):
        assert line["steps"] == 3 and line["warmup"] == 1 and len(line["step_ms"]) == 3 and line["ms_per_step"] > 0
        assert line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert plain["full"] is False and full["full"] is True
    for key in ("profiled_region", "roofline", "step_flops", "tracker_overhead", "bf16_configs2", "cpu_baseline"):
        assert plain[key] is None, key
    assert plain["kernels"] == {}
    assert full["profiled_region"]["steps"] == 3 and full["roofline"]["kernel"] and full["kernels"]
    assert full["tracker_overhead"]["steps_per_arm"] > 0
    assert full["bf16_configs2"] is None and full["cpu_baseline"] is None
