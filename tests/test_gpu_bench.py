"""bench.py on a small map: a plain run reports what its timed steps measured and nothing else; `--full` adds the measurements that
need runs of their own (at sizes other than 720p: `reference_call` and the per-family kernel times)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "4", "--warmup", "1", "--height", "100", "--width", "120"]
FULL_ONLY = ("reference_call", "bf16_letter", "f32_grade", "harness", "train", "cpu_baseline")


def bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "bench.py", *SMALL, *extra], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_reports_the_timed_steps_alone(tmp_path):
    d = bench("--dump-outputs", str(tmp_path))
    assert d["metric"] == "deblurred 720p frames/sec" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["steps"] == 4 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"])
    assert [k for k in FULL_ONLY if k in d] == []
    assert d["roofline"]["families"] == {} and d["roofline"]["kernel"] is None
    assert d["roofline"]["correlation_kernel"]["launch_ms"] > 0          # timed live inside the timed steps
    out = np.load(tmp_path / "output.npy")
    assert d["dump_outputs"]["shapes"] == {"output": [1, 3, 100, 120]} and out.shape == (1, 3, 100, 120)
    assert np.isfinite(out).all()


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements():
    d = bench("--full", "--cpu-baseline", "none")
    assert d["value"] > 0 and d["reference_call"]["value"] > 0
    fams = d["roofline"]["families"]
    assert {"conv", "swin", "correlation"} <= set(fams) and all(f["ms_per_frame"] > 0 for f in fams.values())
    assert d["roofline"]["kernel"] is not None
    assert "cpu_baseline" not in d                                        # --cpu-baseline none still skips it under --full
