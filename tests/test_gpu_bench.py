"""bench.py's plain run (`--gpus 1 --steps K --warmup W`) times both halves of the metric and measures nothing else; what takes runs of its
own — CPU baselines, variants, the edit GEMM roofline, the multi-view record — waits for `--full` (run at N = 2 by
tests/test_gpu_dp_two_ranks.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_metric_only(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dump = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(dump)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["metric"] == "training rays/s" and rec["value"] > 0 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["roofline"]["launches"] > 0                               # event pairs around the timed steps' own gather launches
    assert "variants" not in rec and "cpu_baseline" not in rec
    sec = rec["secondary"]
    assert sec["metric"] == "SDS edit-steps/s" and sec["value"] > 0 and sec["steps"] == 2
    assert not {"roofline", "cpu_baseline", "multi_view"} & set(sec)
    names = set(os.listdir(dump))
    assert {"recon_loss.npy", "edit_loss.npy"} <= names and any(n.startswith("edit_param_") for n in names)
