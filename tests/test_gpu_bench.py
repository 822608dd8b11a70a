"""`bench.py` as it is run for every change: a plain run (no --full) prints the headline line and nothing beside it, and
--dump-outputs writes what the last timed step returned, the same from run to run on the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_step_outputs(tmp_path):
    lines, dumps = [], []
    for i in range(2):
        out_dir = tmp_path / f"run{i}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--images", "1",
               "--proposals", "200", "--classes", "80", "--dump-outputs", str(out_dir)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        dumps.append({n: np.load(out_dir / f"{n}.npy") for n in ("scores", "proposal_deltas")})
    for out in lines:
        assert out["unit"] == "proposals/s" and out["higher_is_better"] is True and isinstance(out["dtype"], str)
        assert out["steps"] == 3 and out["full"] is False and out["ms_per_step"] > 0
        assert abs(out["value"] - 200 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
        assert "train" not in out and "cpu_baseline" not in out and "f32_mfma_reference" not in out
        assert out["scopes"]["S1_handwritten_kernels_proposals_per_s"] is None and out["scopes"]["eval_1img"] is None
    a, b = dumps
    assert a["scores"].shape == (200, 81) and a["proposal_deltas"].shape == (200, 4)
    for name in a:
        assert a[name].dtype == np.float32 and np.isfinite(a[name]).all()
        scale = max(1.0, float(np.abs(a[name]).max()))
        assert float(np.abs(a[name] - b[name]).max()) <= 1e-5 * scale, name
