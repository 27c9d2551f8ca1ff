"""`bench.py` on one GPU: a plain run carries the headline line alone; `--full` adds the measurements beyond it."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "outputs_finite")
FULL_ONLY = ("roofline", "aggregate_roofline", "config2_ragged256", "config0_plumbing", "config4_share_bf16_inpaint",
             "f32x6_candidate", "cpu_baseline", "gpu_over_cpu")


def _bench_line(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
                        *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


def _check_headline(out):
    for k in HEADLINE:
        assert k in out, k
    assert out["unit"] == "molecules/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == 1 and out["warmup"] == 1 and out["outputs_finite"] is True
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 64 * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone():
    out = _bench_line()
    _check_headline(out)
    assert not [k for k in FULL_ONLY if k in out]
    assert "probe_fake_2ms_per_molecule" not in out["host_stages"]


@pytest.mark.gpu
def test_full_run_adds_the_rooflines_and_the_host_stage_probe():
    out = _bench_line("--full", "--no-cpu-baseline", "--no-x6-probe", "--no-config0", "--no-config2", "--no-config4")
    _check_headline(out)
    assert out["roofline"]["avg_launch_us"] > 0 and out["aggregate_roofline"]["avg_launch_us"] > 0
    if not out["host_stages"]["rdkit"]:
        assert "probe_fake_2ms_per_molecule" in out["host_stages"], out["host_stages"]
