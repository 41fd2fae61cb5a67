"""bench.py's options around the headline, CPU only: --dump-outputs writes the last step's cells and proofs as float32 byte values on
a seeded sample no larger than 64 MB, the same for the same batch size, and the argument checks refuse what cannot be timed."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    cells = torch.randint(0, 256, (B * bench.CELLS * bench.BYTES_PER_CELL,), dtype=torch.uint8, generator=g)
    proofs = torch.randint(0, 256, (B * bench.CELLS * 48,), dtype=torch.uint8, generator=g)
    return cells, proofs


def test_dump_outputs_writes_every_blob_of_a_small_batch(tmp_path):
    B = 5
    cells, proofs = _outputs(B, 1)
    bench.dump_outputs(str(tmp_path), cells, proofs, B)
    c, p = np.load(tmp_path / "cells.npy"), np.load(tmp_path / "proofs.npy")
    assert c.dtype == np.float32 and c.shape == (B, 128, 2048)
    assert p.dtype == np.float32 and p.shape == (B, 128, 48)
    assert np.array_equal(c.reshape(-1), cells.numpy()) and np.array_equal(p.reshape(-1), proofs.numpy())


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(tmp_path):
    B = 1100
    cells, proofs = _outputs(B, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), cells, proofs, B)
    total = 0
    for name, per_blob, src in (("cells", bench.CELLS * bench.BYTES_PER_CELL, cells), ("proofs", bench.CELLS * 48, proofs)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b)
        k = bench.DUMP_BLOBS[name]
        assert a.shape[0] == k < B
        idx = np.sort(np.random.RandomState(bench.DUMP_SEED).choice(B, k, replace=False))
        assert np.array_equal(a.reshape(k, -1), src.view(B, per_blob).numpy()[idx])
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total <= 64 * 10**6


def test_steps_and_strong_configs_are_checked_before_any_work():
    for extra, msg in ((["--steps", "0"], "--steps must be at least 1"), (["--strong-configs"], "--strong-configs is a leg of a --full run")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-2000:]
