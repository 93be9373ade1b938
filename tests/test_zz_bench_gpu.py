"""The plain bench line (no --full): the timed steps and the headline alone, and --dump-outputs writing what the last timed step computed
(from the seeded initial state), the same from run to run on the same arguments.  Sorts behind the numerical tests: it starts child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch-per-gpu", "4", "--size", "128",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[:3000], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_its_dumped_outputs(dev, tmp_path):
    runs = [(_bench(tmp_path / d), tmp_path / d) for d in ("a", "b")]
    for d, _ in runs:
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "images/sec" and d["higher_is_better"] is True
        assert d["dtype"] in ("bf16", "fp16") and d["metric"].startswith("640x640 images/sec")
        assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 1e-2 * d["value"]
        for leg in ("repeats", "roofline", "kernels", "event_recording", "strong", "strong16", "eval", "target_encode", "cpu_baseline"):
            assert leg not in d, leg                      # --full only
    (_, a), (_, b) = runs
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) == ["gradients.npy", "l2.npy", "loss_face.npy", "momenta.npy", "weights.npy"]
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.isfinite(x).all(), n
        assert np.allclose(x, y, rtol=1e-5, atol=1e-5 * max(1e-30, float(np.abs(x).max()))), n     # rounding: fp32 atomic order
    loss = np.load(a / "loss_face.npy")
    assert loss.shape == (4,) and loss[3] > 0 and loss[3] == np.load(b / "loss_face.npy")[3]      # positives: the same targets
    w = np.load(a / "weights.npy")
    assert w.ndim == 1 and w.shape == np.load(a / "gradients.npy").shape == np.load(a / "momenta.npy").shape and np.abs(w).max() > 0
