"""A plain `bench.py` run does the headline measurement and nothing else; the extras (roll-out-only leg, CPU baselines, child counter passes,
child runs of the other configurations) run only under `--full`."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_full_is_an_option_of_every_run(capsys):
    had = "HSA_ENABLE_IPC_MODE_LEGACY" in os.environ
    import bench
    if not had:                     # (bench.py sets it for the ranks it starts; this process keeps its own environment)
        os.environ.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)
    bench.main(["--full", "--steps", "2", "--warmup", "1", "--dry-run-ranks"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["metric"] == "dry-run-ranks" and line["steps"] == 2 and line["warmup"] == 1


@pytest.mark.gpu
def test_plain_run_prints_the_headline_without_the_extras(tmp_path):
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path / "d")],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-3000:]
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE_KEYS), sorted(out)
    assert out["steps"] == 1 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["dumped_outputs"]["arrays"] == len(list((tmp_path / "d").glob("*.npy"))) > 0
    # nothing of --full: no CPU baseline, no MJX probe, no child runs of other configurations, no roll-out-only leg, no counters of its own
    assert "cpu_baseline" not in out and "mjx_cpu" not in out and "other_configs" not in out["config"]
    assert out["config"]["rollout_only_env_steps_per_s_per_gpu"] is None and out["roofline"]["avg_launch_ms_isolated"] is None
    assert out["roofline"]["traffic_collected_by_this_run"] is False and out["roofline_mfma"]["mfma_util_collected_by_this_run"] is False
