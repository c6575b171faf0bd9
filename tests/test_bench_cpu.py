"""bench.py --dump-outputs on host tensors: an array above its share of the size budget is cut to a seeded sample of whole items
in ascending order (the same items on every call), one below it is written whole; more than one rank splits the budget."""
import numpy as np
import torch

import bench


def test_dump_outputs_samples_whole_items(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1000)
    items, per_item = 100, 8
    c = torch.arange(items * per_item, dtype=torch.float32)
    bench.dump_outputs(torch, str(tmp_path / "a"), {"c": (c, per_item)}, 0, 1)
    bench.dump_outputs(torch, str(tmp_path / "b"), {"c": (c, per_item)}, 0, 1)
    a, b = np.load(tmp_path / "a" / "c.npy"), np.load(tmp_path / "b" / "c.npy")
    assert a.dtype == np.float32 and a.shape == (1000 // (per_item * 4), per_item)
    assert np.array_equal(a, b)                                          # a fixed sample
    first = a[:, 0].astype(np.int64)
    assert np.all(first % per_item == 0) and np.all(np.diff(first) > 0)  # whole items, ascending, no repeats
    assert np.array_equal(a, c.view(items, per_item).numpy()[first // per_item])
    # two ranks: each writes <name>_rank<r>.npy within half the budget
    bench.dump_outputs(torch, str(tmp_path / "r"), {"c": (c, per_item)}, 1, 2)
    assert np.load(tmp_path / "r" / "c_rank1.npy").shape == (500 // (per_item * 4), per_item)
    # below the budget: the whole array, float64 kept
    small = torch.linspace(-1.0, 1.0, 60, dtype=torch.float64)
    bench.dump_outputs(torch, str(tmp_path / "s"), {"c": (small, 1)}, 0, 1)
    s = np.load(tmp_path / "s" / "c.npy")
    assert s.dtype == np.float64 and np.array_equal(s[:, 0], small.numpy())
