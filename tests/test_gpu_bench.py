"""bench.py's plain run on the device: the headline only, the line's contract keys, and outputs that two runs with the same
arguments reproduce.  Needs an MI355X:  python -m pytest tests -m gpu"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--batch", "2", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_times_the_headline_and_dumps_reproducible_outputs(tmp_path):
    line = _plain_run(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["unit"] == "frames/s"
    assert line["ms_per_step"] > 0 and abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    # the secondary legs are --full's: no roofline pass, CPU baseline, fitting step or detail file in a plain run
    for key in ("roofline", "cpu_baseline", "train_step_ms", "value_fp32_exact", "detail"):
        assert key not in line, key
    shapes = {"image": (2, 3, 512, 512), "image_raw": (2, 3, 128, 128), "image_depth": (2, 1, 128, 128)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in shapes)
    first = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in shapes}
    for k, shape in shapes.items():
        assert first[k].dtype == np.float32 and first[k].shape == shape and np.isfinite(first[k]).all(), k
    assert np.abs(first["image"]).max() > 0.05
    # same arguments, same inputs: the renderer's uniforms drawn inside the timed steps are seeded, whatever `settle` took
    _plain_run(tmp_path / "b")
    for k in shapes:
        again = np.load(tmp_path / "b" / f"{k}.npy")
        assert np.abs(again - first[k]).max() <= 1e-4 * max(1.0, float(np.abs(first[k]).max())), k
