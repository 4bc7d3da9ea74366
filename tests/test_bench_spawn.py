"""bench.py --gpus N from a plain invocation: the parent starts N ranks itself (no torchrun), and a job whose size differs
from --gpus fails instead of degrading (the metric is reported at 1, 2, 4 and 8 GPUs)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH, *args], env=env, capture_output=True, text=True, timeout=300)


def test_plain_invocation_spawns_n_ranks():
    r = _run(["--gpus", "3", "--spawn-check"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.strip().splitlines()) == 1, r.stdout     # ONE JSON line: gloo's connection banners go to stderr
    line = json.loads(r.stdout)
    assert line["n_gpus"] == 3 and line["dist_world_size"] == 3
    assert line["rank_sum"] == 6.0                      # every rank took part in the collective: 1 + 2 + 3
    assert line["launcher"] == "bench.py"


def test_external_launcher_is_respected():
    r = _run(["--gpus", "1", "--spawn-check"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["launcher"] == "external"


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "4", "--spawn-check"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "refusing" in r.stderr
    r = _run(["--gpus", "1", "--spawn-check"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0


def test_a_failing_rank_fails_the_job():
    # rank 1 exits before the rendezvous: the launcher must take the other rank down (it would wait in the collective) and fail
    r = _run(["--gpus", "2", "--spawn-check"], {"B4D_BENCH_TEST_FAIL_RANK": "1"})
    assert r.returncode != 0 and "ranks failed" in r.stderr
    assert "spawn_check" not in r.stdout


def test_plain_run_is_headline_only_and_dumps_are_reproducible(tmp_path):
    # a plain run leaves the secondary legs and the CPU baseline to --full; --dump-outputs writes float32 .npy files, the same
    # bytes for the same outputs, and stays under 64 MB at the default stack (checked here on CPU tensors: no GPU)
    code = f"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, {ROOT!r})
import bench
plain, full = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"]), bench.parse_args(["--full"])
g = torch.Generator().manual_seed(5)
psd, ac = torch.rand((3, 64, 64), generator=g), torch.rand((3, 64, 64), generator=g)
a = bench.dump_outputs(torch, {str(tmp_path / "a")!r}, psd, ac)
b = bench.dump_outputs(torch, {str(tmp_path / "b")!r}, psd, ac)
same = all(np.load(x).tobytes() == np.load(y).tobytes() for x, y in zip(a, b))
dtypes = sorted({{str(np.load(x).dtype) for x in a}})
frame0 = np.array_equal(np.load(a[0]), psd[0].numpy())
default_bytes = 2 * 4 * bench.N * bench.N + 2 * 4 * min(bench.DUMP_SAMPLE, bench.FRAMES_PER_GPU * bench.N * bench.N)
print(json.dumps({{"plain_full": plain.full, "full": full.full, "steps": plain.steps, "dump": plain.dump_outputs,
                  "names": [os.path.basename(x) for x in a], "same": same, "dtypes": dtypes, "frame0": frame0,
                  "default_bytes": default_bytes}}))
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["plain_full"] is False and d["full"] is True and d["steps"] == 3 and d["dump"] is None
    assert sorted(d["names"]) == ["autocorr_frame0.npy", "autocorr_sample.npy", "psd_frame0.npy", "psd_sample.npy"]
    assert d["same"] and d["dtypes"] == ["float32"] and d["frame0"]
    assert d["default_bytes"] <= 64 * 10**6


def test_steps_must_be_positive():
    r = _run(["--gpus", "1", "--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr
