"""A plain ``bench.py`` run at a small batch, as a fresh child process: it times exactly --steps steps, prints the headline fields and none of
what --full measures, and --dump-outputs writes the last step's loss and every trainable parameter's gradient within the 64 MB budget."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_plain_bench_run_dumps_the_last_steps_outputs(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=540)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    for key in ("board_power", "with_optimizer_step", "with_fp32_tower", "cpu_baseline", "other_configs"):
        assert key not in d, key
    assert "dominant_kernel" not in d["roofline"] and "power_capped_pipe" not in d["roofline"]
    files = sorted(os.listdir(out))
    assert "loss.npy" in files and "grad_norms.npy" in files
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    loss = np.load(out / "loss.npy")
    assert loss.dtype == np.float64 and abs(float(loss[0]) - d["loss"]) < 1e-4
    grads = [f for f in files if f.startswith("grad.")]
    assert "grad.llm.emb_dict.weight.npy" in grads and any(f.startswith("grad.adapter.") for f in grads)
    norms = np.load(out / "grad_norms.npy")
    assert norms.shape == (len(grads),) and np.isfinite(norms).all() and (norms > 0).any()
    for f in grads:
        g = np.load(out / f)
        assert g.dtype == np.float32 and np.isfinite(g).all(), f
