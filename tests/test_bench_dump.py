"""bench.py --dump-outputs: the files it writes from a step's result -- float64, the same from call to call, a
bounded sample of a long id list, the whole of a short one. CPU only: the result is a stand-in with host tensors."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _result(n_buf, n_kept):
    ids = torch.arange(0, 3 * n_buf, 3, dtype=torch.int64)          # the caller's buffer: n_kept valid ids, then slack
    return types.SimpleNamespace(kept_read_ids=ids, n_kept=n_kept, n_unique=n_kept + 7, n_edges=11, n_clusters=n_kept)


def test_dump_is_whole_below_the_cap_and_repeatable(tmp_path):
    import bench
    res = _result(5000, 4000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, False, 0, 1)
    assert sorted(os.listdir(tmp_path / "a")) == ["counters.npy", "kept_read_ids.npy"]
    kept, counters = np.load(tmp_path / "a" / "kept_read_ids.npy"), np.load(tmp_path / "a" / "counters.npy")
    assert kept.dtype == np.float64 and counters.dtype == np.float64
    assert np.array_equal(kept, np.arange(0, 12000, 3))             # the valid ids only, none of the slack
    assert counters.tolist() == [4007, 11, 4000, 4000, 4000, float(3 * 4000 * 3999 // 2)]
    for name in ("counters.npy", "kept_read_ids.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))


def test_dump_samples_a_long_list_at_fixed_positions(tmp_path, monkeypatch):
    import bench
    assert bench.DUMP_IDS * 8 + 6 * 8 <= 64 << 20                   # what one rank writes at the most
    monkeypatch.setattr(bench, "DUMP_IDS", 1000)
    res = _result(60000, 50000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, False, 0, 1)
    kept = np.load(tmp_path / "a" / "kept_read_ids.npy")
    assert kept.shape == (1000,) and np.all(np.diff(kept) >= 0) and kept.max() < 150000 and np.all(kept % 3 == 0)
    assert np.array_equal(kept, np.load(tmp_path / "b" / "kept_read_ids.npy"))
    assert np.load(tmp_path / "a" / "counters.npy")[4:].tolist() == [50000, float(3 * 50000 * 49999 // 2)]


def test_a_sharded_rank_writes_its_own_files(tmp_path):
    import bench
    res = _result(100, 100)
    res.n_kept = 250                                                # job-wide; this rank lists its own 100
    bench.dump_outputs(str(tmp_path), res, True, 1, 2)
    assert sorted(os.listdir(tmp_path)) == ["counters_rank1.npy", "kept_read_ids_rank1.npy"]
    assert np.load(tmp_path / "kept_read_ids_rank1.npy").shape == (100,)
