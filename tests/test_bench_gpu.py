"""bench.py's command line: the result line's fields, ``--steps`` timing
exactly that many steps, ``--dump-outputs`` and ``--full`` (one tiny model,
one process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_result_line_and_dump_outputs(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
           "--warmup", "3", "--model", "gpt-tiny", "--seq", "128", "--per-gpu-seqs", "2",
           "--full", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    res = json.loads(lines[0])
    assert res["unit"] == "tokens/s" and res["higher_is_better"] is True
    assert res["dtype"] == "bf16" and res["steps"] == 2 and res["warmup"] == 3
    assert res["config"]["hip_graph"] is True
    # value = tokens of the timed steps / their time; ms_per_step = that time / steps
    # (both rounded in the line: 0.01 ms and 0.1 tokens/s)
    tokens_per_step = 2 * 128
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(tokens_per_step / (res["ms_per_step"] * 1e-3), rel=2e-2)
    loss = np.load(out / "loss.npy")
    assert loss.dtype == np.float64 and loss.shape == (1,) and np.isfinite(loss).all()
    assert float(loss[0]) == pytest.approx(res["final_loss"], abs=1e-4)
    params = np.load(out / "params_sample.npy")
    assert params.dtype == np.float32 and params.ndim == 1 and np.isfinite(params).all()
    assert 0 < params.nbytes <= 64 * 2 ** 20 and np.abs(params).max() > 0
    assert sorted(p.name for p in out.iterdir()) == ["loss.npy", "params_sample.npy"]
