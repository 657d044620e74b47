"""CPU: bench.py --dump-outputs writes float32 arrays, full where they fit their share of the budget
and the same seeded row sample on every call where they do not; --full and --dump-outputs parse."""
import os
import sys
import types

import numpy as np
import torch

import bench


def _last(n_jobs, V, E, B, h, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(types.SimpleNamespace(node_feats=torch.randn(V, h, generator=g),
                                   edge_feats=torch.randn(E, h, generator=g).to(torch.bfloat16)),
             torch.randn(B, h, generator=g)) for _ in range(n_jobs)]


def test_dump_small_outputs_are_written_whole(tmp_path):
    last = _last(1, V=37, E=80, B=5, h=12)
    bench.dump_outputs(last, str(tmp_path / "d"), types.SimpleNamespace(rank=0, world_size=1))
    assert sorted(os.listdir(tmp_path / "d")) == ["edge_feats.npy", "node_feats.npy", "readout.npy"]
    Gout, out = last[0]
    for name, t in (("readout", out), ("node_feats", Gout.node_feats), ("edge_feats", Gout.edge_feats)):
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.float().numpy())


def test_dump_large_outputs_are_a_fixed_row_sample_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 << 10)
    env = types.SimpleNamespace(rank=1, world_size=2)
    last = _last(2, V=900, E=2000, B=40, h=16)
    for d in ("a", "b"):
        bench.dump_outputs(last, str(tmp_path / d), env)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert "rank1_readout_shard0.npy" in files and "rank1_edge_feats_shard1_rows.npy" in files
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        total += a.nbytes
    assert total <= (64 << 10) * 9 // 8  # the budget, plus the row numbers (8 B beside a 64 B row)
    rows = np.load(tmp_path / "a" / "rank1_node_feats_shard1_rows.npy").astype(np.int64)
    assert (np.diff(rows) > 0).all() and rows.max() < 900
    a = np.load(tmp_path / "a" / "rank1_node_feats_shard1.npy")
    assert np.array_equal(a, last[1][0].node_feats[torch.from_numpy(rows)].numpy())


def test_full_and_dump_outputs_parse(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
