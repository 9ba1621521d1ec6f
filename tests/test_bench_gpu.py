"""bench.py's plain run on the GPU: the headline workload only, and --dump-outputs of what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_dumps_the_last_timed_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=540, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "volumes/s"
    assert out["roofline"] is None and "others" not in out and "cpu_baseline" not in out
    arrays = out["outputs"]["arrays"]
    assert set(arrays) == {"out", "model_params", "model_grad", "ema_model_params"}      # unet_3D: InstanceNorm, no buffers
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
    for name, info in arrays.items():
        a = np.load(d / f"{name}.npy")
        assert str(a.dtype) == info["dtype"] in ("float32", "float64") and a.size == info["elements"] <= info["of"]
        assert np.isfinite(a).all(), name
    assert np.load(d / "model_grad.npy").any() and np.load(d / "ema_model_params.npy").any()
    scal = np.load(d / "out.npy")
    assert abs(float(scal[0]) - out["losses_last_step"]["loss"]) <= 1e-5     # the losses of the same (last timed) step
