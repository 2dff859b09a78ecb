"""bench.py's plain run on the GPU: the headline only (every context field null), --steps sets the timed steps, and --dump-outputs
writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    dump = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--prewarm-s", "0",
           "--prewarm-steps", "2", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["config"]["full"] is False
    assert line["ms_per_step"] > 0 and line["unit"] == "rays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    # value = the 7 timed steps' rays over their time, ms_per_step = that time / 7 (rounded to 4 decimals)
    assert abs(1024 / (line["ms_per_step"] * 1e-3) / line["value"] - 1) < 1e-3
    for key in ("roofline", "colour_gather", "cpu_baseline", "reference_shaped_gpu", "dropin", "mapping_iteration", "precision_modes",
                "small_shapes"):
        assert line[key] is None, key

    arrays = {p.name[:-4]: np.load(p) for p in dump.glob("*.npy")}
    assert set(arrays) == {"loss", "camera", "pose_grad", "candidate_camera", "min_loss", "ray_l1"}
    shapes = {"loss": (1,), "camera": (7,), "pose_grad": (7,), "candidate_camera": (7,), "min_loss": (1,), "ray_l1": (1024,)}
    for name, a in arrays.items():
        assert a.dtype == np.float32 and a.shape == shapes[name] and np.isfinite(a).all(), name
    assert abs(float(arrays["loss"][0]) - line["final_loss"]) <= 1e-6
    # the loss is the per-ray L1 sums over 3 R; the Adam step moved the camera along a non-zero gradient
    assert np.isclose(arrays["ray_l1"].sum(dtype=np.float64) / (3 * 1024), arrays["loss"][0], rtol=1e-5)
    assert np.abs(arrays["pose_grad"]).max() > 0
    assert arrays["min_loss"][0] <= arrays["loss"][0]
