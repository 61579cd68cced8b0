"""bench.py end to end on the GPU: a plain run's result line and the arrays
--dump-outputs writes, against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bitexact, flat_from_export, oracle_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_timed_steps_image(gpu, pt_mod, oracle_mod, tmp_path):
    """bench.py --steps 3 --dump-outputs on a small frame: the line reports 3
    steps with ms_per_step and none of the --full measurements, and image.npy is
    the accumulator of exactly the 3 timed iterations (ids 0..2; the warmup's
    iteration is cleared), bit for bit the oracle's."""
    from pathtracerap_amd import synthetic
    P, O = pt_mod, oracle_mod
    out = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--ntri", "3000", "--width", "96", "--height", "72", "--dump-outputs", out],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, p.stdout
    d = json.loads(line[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["full"] is False and d["config"]["trace_faults"] == 0
    for key in ("full_run", "roofline", "cpu_baseline", "alt_mode", "targets"):
        assert d[key] is None, key
    got = np.load(os.path.join(out, "image.npy"))
    assert got.dtype == np.float32 and got.shape == (72, 96, 3)
    s = P.Scene(synthetic.diffuse_scene(str(tmp_path / "scene"), ntri=3000, width=96, height=72))
    cfg = s.apply_settings(P.RenderConfig())
    cfg.width, cfg.height, cfg.iterations, cfg.accel = 96, 72, 3, P.ACCEL_GRID_FAST
    s.build(grid=cfg.grid, bvh=True)
    want, seg = O.render(flat_from_export(s.export(), cfg.grid), oracle_cfg(cfg, threads=4))
    assert np.abs(got).sum() > 0
    assert_bitexact(got.reshape(-1, 3), want.reshape(-1, 3), "bench image")
    counts = np.load(os.path.join(out, "segments_per_bounce.npy"))
    assert counts.dtype == np.float64 and counts.sum() == seg == d["config"]["segments"]
