"""bench.py's options around the timed steps, at a tiny size on the CPU engine: a plain run reports the
requested steps and ``ms_per_step`` and leaves the holdout AUC to ``--full``; ``--dump-outputs`` writes the
last fit's model as float arrays that two runs with the same arguments reproduce exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--device", "cpu",
                          "--rows", "5000", "--iterations", "3", "--steps", "2", "--warmup", "1", *extra],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_identical_outputs(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "a"))
    full = _bench("--full", "--dump-outputs", str(tmp_path / "b"))
    for rec in (plain, full):
        assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
        assert rec["higher_is_better"] is True and rec["dtype"] == "fp32"
        # value = rows x steps / seconds of the timed steps, ms_per_step = those seconds / steps (both rounded)
        assert rec["value"] == pytest.approx(5000 / (rec["ms_per_step"] / 1e3), rel=1e-3)
    assert plain["config"]["holdout_auc"] is None
    assert 0.5 < full["config"]["holdout_auc"] <= 1.0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "leaf_value.npy" in names and "threshold.npy" in names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.size > 0
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "num_leaves.npy").shape == (3,)  # one entry per tree of the 3-iteration fit
    assert np.load(tmp_path / "a" / "holdout_probability.npy").shape == (5000,)
