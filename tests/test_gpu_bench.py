"""GPU: bench.py's plain line and --dump-outputs on a small geometry.  Two runs with the same arguments hand the same
inputs to every step and write the same outputs (to the rounding of one step: warp, loss and NCE reductions still meet in
fp32 atomics); the plain line carries the headline fields and none of the --full measurements."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "3", "--batch", "2",
           "--size", "64", "--ngf", "8", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_plain_line_and_reproducible_dump(tmp_path):
    a, b = _bench(str(tmp_path / "a")), _bench(str(tmp_path / "b"))
    for r in (a, b):
        assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["higher_is_better"] is True
        assert abs(r["value"] - 2 * r["steps"] / (r["ms_per_step"] * 1e-3 * r["steps"])) < 1e-6 * r["value"]
        assert not ({"roofline", "roofline_hbm", "also_3d", "also_3d_128", "cpu_baseline", "value_host_inputs"} & set(r))
    fa = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "a" / "*.npy")))
    fb = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "b" / "*.npy")))
    assert fa == fb and "visual_fake_B.npy" in fa and "loss_G.npy" in fa
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in fa) <= 64 << 20
    for f in fa:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == (np.float64 if f.startswith("loss_") else np.float32), f
        assert np.isfinite(x).all(), f
        assert np.allclose(x, y, rtol=1e-5, atol=1e-6 * max(float(np.abs(x).max()), 1e-30)), f
