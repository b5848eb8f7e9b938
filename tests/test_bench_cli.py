"""bench.py command-line contract on the CPU path: --steps sets the timed
step count, the result line carries ms_per_step, --dump-outputs writes a
reproducible float32 output of the last timed step, --full is accepted."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*extra):
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--device", "cpu",
         "--size", "64", "--warmup", "1", *extra],
        capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("mode,steps", [("replicated", 2), ("blockrow", 3)])
def test_dump_outputs_reproducible(tmp_path, mode, steps):
    """Two runs with the same arguments dump identical arrays, whatever
    --steps is (the last step starts from a seeded C)."""
    dumps = []
    for d, st in (("a", steps), ("b", steps), ("c", 1)):
        j = _run_bench("--steps", str(st), "--mode", mode, "--full",
                       "--dump-outputs", str(tmp_path / d))
        assert j["steps"] == st
        assert j["ms_per_step"] > 0
        assert j["dtype"] == "fp32" and j["higher_is_better"] is True
        assert os.listdir(tmp_path / d) == ["c.npy"]
        dumps.append(np.load(tmp_path / d / "c.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (64, 64)
    assert np.isfinite(dumps[0]).all() and np.abs(dumps[0]).max() > 0
    assert np.array_equal(dumps[0], dumps[1])
    assert np.array_equal(dumps[0], dumps[2])


def test_dump_output_row_sample(tmp_path, monkeypatch):
    """Above the size cap the dump is a fixed sample of whole rows."""
    import bench
    monkeypatch.setattr(bench, "_DUMP_MAX_BYTES", 10 * 32 * 4)
    t = torch.arange(64 * 32, dtype=torch.float32).view(64, 32)
    bench.dump_output(str(tmp_path), "c", t)
    bench.dump_output(str(tmp_path), "c2", t)
    got = np.load(tmp_path / "c.npy")
    assert got.dtype == np.float32 and got.shape == (10, 32)
    assert np.array_equal(got, np.load(tmp_path / "c2.npy"))
    rows = (got[:, 0] / 32).astype(int)
    assert len(set(rows)) == 10 and list(rows) == sorted(rows)
    assert np.array_equal(got, t.numpy()[rows])
    # at or below the cap the whole matrix is written
    bench.dump_output(str(tmp_path), "small", t[:10])
    assert np.array_equal(np.load(tmp_path / "small.npy"), t[:10].numpy())
