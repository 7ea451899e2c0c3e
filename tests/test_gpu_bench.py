"""A plain bench.py run: exactly --steps timed steps in one window, the headline fields only, and --dump-outputs writes what
the last timed step left to its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(built_lib, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 7 and len(out["windows_ms_per_step"]) == 1 and out["ms_per_step"] > 0
    assert "roofline" not in out and "cpu_baseline" not in out
    cost = np.load(str(tmp_path / "cost.npy"))
    assert cost.dtype == np.float64 and cost.shape == (1,) and cost[0] == out["final_cost"]
    for name, shape in (("W", (4096, 1024)), ("hbias", (1024,)), ("vbias", (4096,)),
                        ("W_speed", (4096, 1024)), ("hbias_speed", (1024,)), ("vbias_speed", (4096,))):
        a = np.load(str(tmp_path / (name + ".npy")))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), name
