"""bench.py --dump-outputs: the last timed step's output as float32 .npy, a fixed seeded sample of the streams above the cap (CPU only)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_is_the_whole_output_below_the_cap(tmp_path):
    y = torch.randn((1, 256, 2, 1024), dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "d"), y)
    a = np.load(tmp_path / "d" / "y.npy")
    assert a.dtype == np.float32 and np.array_equal(a, y.numpy())


def test_dump_above_the_cap_is_the_same_sample_of_whole_streams(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 1 << 20)
    y = torch.randn((2, 300, 2, 1024), dtype=torch.float32)              # 4.7 MB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), y)
    a, b = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert np.array_equal(a, b) and a.dtype == np.float32
    assert 0 < a.nbytes <= 1 << 20 and a.shape[0] == 2 and a.shape[2:] == (2, 1024)
    # every kept stream is one of y's, whole, in stream order
    idx = [int(np.flatnonzero((y.numpy()[0] == a[0, k]).all(axis=(1, 2)))[0]) for k in range(a.shape[1])]
    assert idx == sorted(set(idx))
    assert np.array_equal(a, y.numpy()[:, idx])
