"""-m gpu: `bench.py --gpus 1 --steps K --warmup W` without --full is the headline measurement alone: it times exactly K steps, and
`--dump-outputs DIR` writes what the last timed step returned -- the same array for the same flags, whatever K is."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "decode_out.npy"))


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_its_output(tmp_path):
    rec, y = _run(tmp_path / "a", 7)
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) <= 1e-3 * rec["value"]   # one token per step and rank
    assert "extra" not in rec and rec["cpu_baseline"] is None and rec["sustained"] is None and rec["roofline"]["traffic"] is None
    assert y.dtype == np.float32 and y.shape == (1, 4096) and np.isfinite(y).all() and np.abs(y).max() > 0
    _, y2 = _run(tmp_path / "b", 3)
    assert np.array_equal(y, y2)
