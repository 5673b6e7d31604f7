"""bench.py --dump-outputs on host tensors (no GPU): what the timed step returned comes back exactly from the float64 files,
the sampled rows are the same on every run, and the files stay under 64 MB whatever the shard size."""
import os

import numpy as np
import torch

import bench


def _outputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 72), dtype=torch.int64, generator=g)
    ok = (torch.rand(n, generator=g) < 0.01).to(torch.uint8)
    return gt, ok, torch.tensor([0], dtype=torch.int32)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_round_trips_exactly_on_fixed_rows(tmp_path):
    n = 1 << 15
    gt, ok, flag = _outputs(n, 1)
    bench.dump_outputs(str(tmp_path / "a"), gt, ok, flag)
    bench.dump_outputs(str(tmp_path / "b"), gt, ok, flag)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["all_ok", "gt", "gt_rows", "ok"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["gt_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_GT_ROWS and len(np.unique(rows)) == len(rows)
    halves = a["gt"].astype(np.uint64).reshape(-1, 72, 2)
    limbs = halves[..., 0] | (halves[..., 1] << np.uint64(32))
    assert np.array_equal(limbs, gt.numpy().view(np.uint64)[rows])
    assert np.array_equal(a["ok"], ok.numpy().astype(np.float64)) and a["all_ok"].tolist() == [0.0]


def test_dump_samples_ok_of_a_large_shard_and_stays_under_64_mb(tmp_path, monkeypatch):
    # the largest dump: DUMP_GT_ROWS Gt rows of 144 halves, DUMP_OK_MAX ok values, the row indices and the flag, 8 bytes each
    assert 8 * (bench.DUMP_GT_ROWS * 145 + bench.DUMP_OK_MAX + 1) < 64 * 10 ** 6
    monkeypatch.setattr(bench, "DUMP_OK_MAX", 1 << 14)
    gt, ok, flag = _outputs(1 << 15, 2)
    bench.dump_outputs(str(tmp_path), gt, ok, flag)
    d = _load(tmp_path)
    rows = d["gt_rows"].astype(np.int64)
    assert np.array_equal(d["ok"], ok.numpy()[rows].astype(np.float64))
