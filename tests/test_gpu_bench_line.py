"""The plain bench.py line (N = 1): the contract keys and nothing that takes runs of its own (those come with --full); --steps sets the
timed steps; --dump-outputs writes the last timed step's output as float32 .npy within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["ms_per_step"] > 0 and res["value"] > 0 and res["unit"] == "edges/s" and res["higher_is_better"] is True
    assert res["dtype"].startswith("f32 in/out")
    assert not {"roofline", "stage_ms_per_step", "cpu_baseline", "configs"} & set(res), sorted(res)
    files = sorted(os.listdir(tmp_path))
    assert files == ["node_features.npy"], files
    out = np.load(tmp_path / "node_features.npy")
    assert out.dtype == np.float32 and out.shape == (16384, 512) and np.isfinite(out).all()
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
