"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run prints the headline line and nothing that needs runs of its own (those
are --full's), and --dump-outputs writes what its last timed step computed -- bitwise the same in a second process (DESIGN.md
section 3: the NeuS training step is reproducible), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "8",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[:400]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_reproducible_outputs(tmp_path):
    a = _bench(tmp_path / "a")
    assert a["metric"] == "training rays/sec" and a["unit"] == "rays/s" and a["higher_is_better"] is True and a["dtype"] == "f32"
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0
    assert abs(a["value"] - a["config"]["rays_per_rank"] / (a["ms_per_step"] * 1e-3)) < 1e-3 * a["value"]
    for k in ("kernels", "roofline", "cpu_baseline", "parity_check", "secondary", "psnr_at_2k", "comm"):
        assert k not in a, k
    b = _bench(tmp_path / "b")
    for name, n in (("stats", 8), ("params", 802491), ("grad", 802491)):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and x.shape == (n,) and np.isfinite(x).all(), name
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert abs(float(np.load(tmp_path / "a" / "stats.npy")[0]) - a["final_stats"]["loss"]) < 1e-4
