"""GPU: a plain `bench.py` run prints the headline line and measures nothing beyond its timed steps."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_prints_only_the_headline_measurement():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - out["config"]["frames_per_step_per_gpu"] / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert "fp32" not in out and "cpu_baseline" not in out and "hbm_families" not in out["roofline"]
    assert out["roofline"]["ranked_over"] == "the LSTM launches of the timed region"
    assert "per-launch pass" not in r.stderr and "CPU baseline" not in r.stderr
    # the whole run, start to exit, spends at most 30 s outside its warm-up and timed steps
    outside = wall - (out["steps"] + out["warmup"]) * out["ms_per_step"] * 1e-3
    assert outside < 30.0, (wall, out["ms_per_step"])
