"""bench.py's two kinds of run: a plain one measures the headline figure alone, `--full` adds everything else."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup")
FULL_ONLY = ("roofline", "roofline_dense", "full_step_cfg4", "full_step_cfg3", "cpu_baseline", "cpu_baseline_1thread",
             "eager_rocm_forward_ms", "eager_rocm_fwd_bwd_ms", "forward_ms", "pemsd4", "widths48", "widths96",
             "widths72_kernels", "dropin_loop", "stress")


def test_full_is_off_by_default():
    import bench
    assert not bench.parse_args([]).full
    assert not bench.parse_args(["--no-baselines"]).full
    args = bench.parse_args(["--full", "--no-baselines", "--steps", "3"])
    assert args.full and args.no_baselines and args.steps == 3


def _bench_line(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]      # stdout carries the one JSON line and nothing else
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    line = _bench_line()
    for key in CONTRACT:
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(32 / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert [k for k in FULL_ONLY if k in line] == []


@pytest.mark.gpu
def test_full_no_baselines_adds_the_rooflines_alone():
    line = _bench_line("--full", "--no-baselines")
    for key in CONTRACT:
        assert key in line, key
    assert line["roofline"]["us_per_launch"] > 0 and line["roofline"]["bound"] == "hbm"
    assert set(line["roofline_dense"]["kernels"]) == {"k_scores", "k_bwd_dense_col"}
    assert [k for k in FULL_ONLY if k in line and not k.startswith("roofline")] == []
