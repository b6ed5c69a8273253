"""CPU: bench.py --dump-outputs stays under its 64 MB budget whatever the number and size of the visuals, writes float32
visuals / float64 losses, keeps small arrays whole and samples large ones at fixed, seeded positions."""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _model(n_big):
    g = torch.Generator().manual_seed(7)
    m = types.SimpleNamespace(visual_names=["small"] + ["big%d" % i for i in range(n_big)] + ["absent"])
    m.small = torch.randn(2, 1, 8, 8, generator=g)
    for i in range(n_big):
        setattr(m, "big%d" % i, torch.randn(16, 1, 512, 512, generator=g))    # 4 Mi elements each
    m.get_current_losses = lambda: {"G": 1.25, "R": 0.5}
    return m


def test_dump_outputs_budget_and_types(tmp_path):
    m = _model(20)
    names = bench.dump_outputs(m, str(tmp_path / "a"))
    assert names == sorted(["loss_G", "loss_R", "visual_small"] + ["visual_big%d" % i for i in range(20)])
    files = [tmp_path / "a" / (n + ".npy") for n in names]
    assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_MAX_BYTES
    small = np.load(tmp_path / "a" / "visual_small.npy")
    assert small.dtype == np.float32 and np.array_equal(small, m.small.numpy())
    loss = np.load(tmp_path / "a" / "loss_G.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [1.25]
    big = np.load(tmp_path / "a" / "visual_big3.npy")
    assert big.dtype == np.float32 and big.ndim == 1 and 0 < big.size <= bench.DUMP_MAX_ELEMS
    assert np.isin(big, m.big3.numpy().reshape(-1)).all()          # a sample of the array's own elements
    bench.dump_outputs(m, str(tmp_path / "b"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))), n


def test_dump_outputs_few_arrays_keep_the_per_array_cap(tmp_path):
    m = _model(2)
    bench.dump_outputs(m, str(tmp_path))
    assert np.load(tmp_path / "visual_big0.npy").size == bench.DUMP_MAX_ELEMS
