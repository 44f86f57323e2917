"""bench.py --dump-outputs on the CPU float32 path: the same arguments give
the same inputs, so two runs write identical arrays."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out, steps):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "1", "--model", "gpt-tiny", "--seq", "32", "--per-gpu-seqs", "2",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


def test_bench_dump_outputs_repeat_and_follow_steps(tmp_path):
    res = [_bench(tmp_path / "a", 2), _bench(tmp_path / "b", 2), _bench(tmp_path / "c", 3)]
    for r, steps in zip(res, (2, 2, 3)):
        assert r["steps"] == steps and r["ms_per_step"] > 0 and r["unit"] == "tokens/s"
    dumps = [{n: np.load(tmp_path / d / (n + ".npy")) for n in ("loss", "params_sample")}
             for d in "abc"]
    for d in dumps:
        assert d["loss"].dtype == np.float64 and d["loss"].shape == (1,)
        assert d["params_sample"].dtype == np.float32 and np.isfinite(d["params_sample"]).all()
    assert np.array_equal(dumps[0]["loss"], dumps[1]["loss"])
    assert np.array_equal(dumps[0]["params_sample"], dumps[1]["params_sample"])
    # one more timed step is one more update: --steps really sets the count
    assert not np.array_equal(dumps[0]["params_sample"], dumps[2]["params_sample"])
