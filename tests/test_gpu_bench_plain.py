"""bench.py run plain (no --full) on one GPU: set-up, warm-up, the timed steps, --dump-outputs and the line -- nothing beside the headline (no side object,
no roofline of launches timed apart, no CPU baseline); --full adds them after the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_headline_only(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "8", "--config", "small", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line: %r" % lines
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "step_roofline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 40 and j["warmup"] == 8 and j["unit"] == "tokens/s" and j["higher_is_better"] is True
    assert abs(j["value"] - 1e3 / j["ms_per_step"]) <= 1e-3 * j["value"]
    assert "side" not in j and "roofline" not in j and j["cpu_baseline"] is None
    assert j["config"]["decode_path"]
    ids, lg = np.load(tmp_path / "ids.npy"), np.load(tmp_path / "logits.npy")
    assert ids.shape == (40,) and lg.shape == (4096,) and np.isfinite(lg).all()
