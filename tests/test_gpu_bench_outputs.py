"""bench.py's plain run and --dump-outputs on the GPU: a plain run prints the headline line
without the --full measurements, and two runs with the same arguments write the same outputs bit
for bit although their clock-settling phases differ in length (--warm-ms 30 against 90: the
settling frames run on a renderer of their own).  Config ref (440x330, mode 1, pipelined as the
flagship config is) keeps the two runs, started side by side, within a few seconds."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["gbuffer_depth.npy", "gbuffer_normals.npy", "gbuffer_pixels.npy", "image.npy"]


@pytest.mark.gpu
def test_plain_runs_dump_identical_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    procs = [subprocess.Popen([sys.executable, "-u", str(ROOT / "bench.py"), "--gpus", "1", "--config", "ref",
                               "--steps", "5", "--warmup", "3", "--warm-ms", ms, "--dump-outputs", str(tmp_path / d)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=str(ROOT))
             for d, ms in (("a", "30"), ("b", "90"))]
    lines = []
    for p in procs:
        out, err = p.communicate(timeout=100)
        assert p.returncode == 0, err[-3000:]
        js = [ln for ln in out.splitlines() if ln.startswith("{")]
        assert len(js) == 1, out[-2000:]
        lines.append(json.loads(js[0]))
    for line in lines:
        assert line["steps"] == 5 and line["warmup"] == 3 and line["full"] is False
        assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        # value and ms_per_step are the same measurement: W * H * spp rays per step (ms_per_step is
        # printed to 1e-4 ms, up to 1% of a frame of this size)
        assert line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(440 * 330 * 4 / line["ms_per_step"] / 1e3, rel=2e-2)
        for key in ("roofline", "roofline_post", "cpu_baseline", "ssbo_path"):  # --full only
            assert key not in line
    for name in NAMES:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.shape == b.shape
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == NAMES
    img = np.load(tmp_path / "a" / "image.npy")
    assert img.shape == (330, 440, 4) and np.nanmax(img[..., :3]) > 0  # a rendered frame
    assert np.load(tmp_path / "a" / "gbuffer_pixels.npy").shape == (440, 64, 4)
