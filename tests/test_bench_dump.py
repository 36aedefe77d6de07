"""bench.py --dump-outputs: the writer of the last timed step's detections (CPU; the GPU run of
the bench itself is tests/test_gpu_bench_dist.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float32_and_zeroes_rows_past_the_count(tmp_path):
    import bench

    g = torch.Generator().manual_seed(0)
    dets = torch.rand((3, 5, 6), generator=g) + 1.0   # no zero anywhere
    counts = torch.tensor([5, 0, 2], dtype=torch.int32)
    keep = dets.clone()
    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(out), dets, counts)
    assert sorted(os.listdir(out)) == ["counts.npy", "dets.npy"]
    d, c = np.load(out / "dets.npy"), np.load(out / "counts.npy")
    assert d.dtype == np.float32 and c.dtype == np.float32
    assert d.shape == (3, 5, 6) and c.tolist() == [5.0, 0.0, 2.0]
    assert np.array_equal(d[0], keep[0].numpy()) and np.array_equal(d[2, :2], keep[2, :2].numpy())
    assert not d[1].any() and not d[2, 2:].any()
    assert torch.equal(dets, keep)   # the caller's tensors are left alone
