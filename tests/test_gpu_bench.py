"""GPU test of bench.py's plain run (pytest -m gpu): without --full it measures the headline alone."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_measures_the_headline_only(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` sets up, warms up, times the K steps, writes --dump-outputs and prints the one
    JSON line with the contract keys; the side measurements that --full adds (roofline step, host enqueue, host-fed loop, the
    other precisions, CPU baseline) do not run: the headline is the only timed measurement in the log."""
    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("images/sec DyT ViT-B/16 fine-tune step") and d["unit"] == "images/s"
    assert d["higher_is_better"] is True and d["dtype"] == "fp16" and d["steps"] == 3 and d["warmup"] == 1
    assert abs(d["value"] - 128 * 1000.0 / d["ms_per_step"]) < 0.01 * d["value"]
    assert abs(d["config"]["keep_ratio_measured"] - 0.7) < 0.02
    for k in ("roofline", "host_enqueue_ms_per_step", "host_fed", "other_fast_mode", "parity_mode", "exact_mode", "cpu_baseline",
              "side_measurement_errors"):
        assert k not in d, k
    timed = [l for l in r.stderr.splitlines() if re.search(r"\] timed \d+ steps:", l)]
    assert len(timed) == 1 and "[fp16/compact] timed 3 steps:" in timed[0], timed
    assert (dump / "losses.npy").is_file() and len(list(dump.glob("param.*.npy"))) > 0
