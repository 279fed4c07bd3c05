"""bench.py as a plain run: the headline line of `--steps` timed steps without the `--full` side figures, and what
`--dump-outputs` writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(gpu, tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--soak", "10",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 6 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "BA-update iters/s" and d["higher_is_better"] is True and d["metric"] and d["dtype"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3          # value = steps / elapsed, ms_per_step = elapsed / steps
    assert d["checks"]["ba_status"][0] == 0 and d["config"]["edges_local"] == 36
    for side in ("burst_value", "sustained_value", "rays_per_sec", "roofline", "cpu_baseline", "sequence"):
        assert side not in d, side                                       # measured with --full only

    shapes = {"poses": (8, 7), "disps": (8, 60, 80), "disps_up": (8, 480, 640), "depth_scale": (8,), "depth_shift": (8,),
              "target": (1, 36, 60, 80, 2), "weight": (1, 36, 60, 80, 2), "net_sample": (1 << 21,)}
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in shapes)
    total = 0
    for name, shape in shapes.items():
        a = np.load(out_dir / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape, (name, a.dtype, a.shape)
        assert np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
