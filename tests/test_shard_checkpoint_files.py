"""Shard files of a row-sharded checkpoint on the host: the writer's layout, and the reader at any row range and number of
writers, with new entities beyond the checkpoint's entity count and the errors of an incomplete checkpoint."""
import os

import numpy as np
import pytest

from openkeonspark_amd import distribute_training as dt


def _write(base, table, world, moments=True):
    """The shard files `world` ranks of a run over `table` would write (chunk = ceil(E / world), as train_paths.setup_shards)."""
    E = table.shape[0]
    chunk = -(-E // world)
    for g in range(world):
        lo, hi = min(g * chunk, E), min((g + 1) * chunk, E)
        extra = dict(adam=table[lo:hi] + 1, adam_1=table[lo:hi] + 2) if moments else {}
        dt._atomic_savez(base + ".shard%dof%d.npz" % (g, world), rows=table[lo:hi], lo=np.int64(lo), hi=np.int64(hi),
                         ent_total=np.int64(E), **extra)


def test_atomic_savez_writes_what_np_load_reads(tmp_path):
    path = str(tmp_path / "a.npz")
    made = []
    big = lambda: made.append(1) or np.arange(12, dtype=np.float32).reshape(3, 4)    # a member produced when it is written
    dt._atomic_savez(path, rows=big, lo=np.int64(3), beta=np.float32(0.9), streams=np.arange(4, dtype=np.uint64))
    with np.load(path) as z:
        assert z.files == ["rows", "lo", "beta", "streams"] and made == [1]
        assert np.array_equal(z["rows"], big()) and int(z["lo"]) == 3 and z["beta"].dtype == np.float32
        assert z["streams"].dtype == np.uint64
    assert os.listdir(str(tmp_path)) == ["a.npz"]      # no temporary left behind


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("key,add", [("rows", 0), ("adam", 1), ("adam_1", 2)])
def test_any_row_range_from_any_number_of_writers(tmp_path, world, key, add):
    table = np.random.default_rng(world).standard_normal((1001, 8)).astype(np.float32)
    base = str(tmp_path / "model.ckpt-7")
    _write(base, table, world)
    parts = dt.shard_files(base, ("rows", "adam", "adam_1"))
    assert parts[1] == 1001 and [p[1] for p in parts[0]] == sorted(p[1] for p in parts[0])
    for lo, hi in ((0, 1001), (0, 334), (333, 668), (500, 501), (1000, 1001), (250, 1001)):
        got, ent_total = dt.read_entity_rows(base, lo, hi, 8, key)
        assert ent_total == 1001 and np.array_equal(got, table[lo:hi] + add)


def test_rows_beyond_the_entity_count_are_new_and_zero(tmp_path):
    table = np.random.default_rng(0).standard_normal((1000, 4)).astype(np.float32)
    base = str(tmp_path / "model.ckpt-5")
    _write(base, table, 2)
    got, ent_total = dt.read_entity_rows(base, 900, 1050, 4)     # a shard of a grown run reaching past the checkpoint
    assert ent_total == 1000 and np.array_equal(got[:100], table[900:]) and not got[100:].any()
    got, _ = dt.read_entity_rows(base, 1050, 2100, 4, "adam")    # a shard of new entities only
    assert got.shape == (1050, 4) and not got.any()


def test_a_missing_shard_file_is_an_error(tmp_path):
    table = np.ones((1000, 4), np.float32)
    base = str(tmp_path / "model.ckpt-5")
    _write(base, table, 4)
    os.remove(base + ".shard2of4.npz")
    with pytest.raises(ValueError, match=r"entity rows \[500, 1000\) are not in any of its shard files"):
        dt.read_entity_rows(base, 0, 250, 4)       # even a range the remaining files hold: the checkpoint is incomplete
    with pytest.raises(ValueError, match="no shard files"):
        dt.shard_files(str(tmp_path / "model.ckpt-6"))


def test_shard_files_without_moments(tmp_path):
    table = np.ones((100, 4), np.float32)
    base = str(tmp_path / "model.ckpt-5")
    _write(base, table, 2, moments=False)          # an SGD checkpoint: rows only, read as before
    assert np.array_equal(dt.read_entity_rows(base, 0, 100, 4)[0], table)
    with pytest.raises(ValueError, match="has no adam, adam_1"):
        dt.shard_files(base, ("rows", "adam", "adam_1"))
    with pytest.raises(ValueError, match="has no adam"):
        dt.read_entity_rows(base, 0, 50, 4, "adam")


def test_shard_files_of_different_entity_counts(tmp_path):
    base = str(tmp_path / "model.ckpt-5")
    _write(base, np.ones((100, 4), np.float32), 2, moments=False)
    dt._atomic_savez(base + ".shard1of2.npz", rows=np.ones((60, 4), np.float32), lo=np.int64(50), hi=np.int64(110),
                     ent_total=np.int64(110))
    with pytest.raises(ValueError, match="different entity counts"):
        dt.shard_files(base)
