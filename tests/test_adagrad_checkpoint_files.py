"""Adagrad accumulators in the shard files of a row-sharded checkpoint, on the host: which arrays a resuming run asks of the
files (`adagrad` present, missing, or not wanted), the reader's fill for new entities, and the whole-table growth
(tests/test_shard_checkpoint_files.py's style; the device side is tests/test_gpu_adagrad_checkpoint.py)."""
import numpy as np
import pytest

from openkeonspark_amd import distribute_training as dt


def _write(base, table, world, adagrad=True):
    E = table.shape[0]
    chunk = -(-E // world)
    for g in range(world):
        lo, hi = min(g * chunk, E), min((g + 1) * chunk, E)
        extra = dict(adagrad=table[lo:hi] + 3) if adagrad else {}
        dt._atomic_savez(base + ".shard%dof%d.npz" % (g, world), rows=table[lo:hi], lo=np.int64(lo), hi=np.int64(hi),
                         ent_total=np.int64(E), **extra)


def test_which_arrays_a_resuming_run_reads():
    adagrad_ckpt = {"rel_embeddings": 0, "rel_embeddings/Adagrad": 0, "global_step": 5}
    adam_ckpt = {"rel_embeddings": 0, "rel_embeddings/Adam": 0, "rel_embeddings/Adam_1": 0, "beta1_power": 0.9, "beta2_power": 0.999}
    sgd_ckpt = {"rel_embeddings": 0, "global_step": 5}
    assert dt.slot_keys(adagrad_ckpt, False, True) == ("rows", "adagrad")
    assert dt.slot_keys(sgd_ckpt, False, True) == ("rows",)              # an SGD checkpoint under Adagrad: fresh accumulators
    assert dt.slot_keys(adagrad_ckpt, False, False) == ("rows",)          # an Adagrad checkpoint under SGD: accumulators ignored
    assert dt.slot_keys(adagrad_ckpt, True, False) == ("rows",)           # ... and under LazyAdam: zero moments
    assert dt.slot_keys(adam_ckpt, False, True) == ("rows",)
    assert dt.slot_keys(adam_ckpt, True, False) == ("rows", "adam", "adam_1")
    assert dt.slot_keys(sgd_ckpt, True, False) == ("rows",)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_accumulator_rows_from_any_number_of_writers(tmp_path, world):
    table = np.random.default_rng(world).standard_normal((1001, 8)).astype(np.float32)
    base = str(tmp_path / "model.ckpt-7")
    _write(base, table, world)
    parts = dt.shard_files(base, ("rows", "adagrad"))
    assert parts[1] == 1001
    for lo, hi in ((0, 1001), (333, 668), (1000, 1001)):
        got, ent_total = dt.read_entity_rows(base, lo, hi, 8, "adagrad", parts, fill=0.1)
        assert ent_total == 1001 and np.array_equal(got, table[lo:hi] + 3)


def test_new_entities_get_the_initial_value(tmp_path):
    table = np.random.default_rng(0).standard_normal((1000, 4)).astype(np.float32)
    base = str(tmp_path / "model.ckpt-5")
    _write(base, table, 2)
    got, ent_total = dt.read_entity_rows(base, 900, 1050, 4, "adagrad", fill=0.1)     # a shard reaching past the checkpoint
    assert ent_total == 1000 and np.array_equal(got[:100], table[900:] + 3)
    assert got.dtype == np.float32 and (got[100:] == np.float32(0.1)).all()
    got, _ = dt.read_entity_rows(base, 1050, 2100, 4, "adagrad", fill=0.1)            # a shard of new entities only
    assert got.shape == (1050, 4) and (got == np.float32(0.1)).all()
    got, _ = dt.read_entity_rows(base, 900, 1050, 4)                                  # rows (and Adam moments) as before: zeros
    assert not got[100:].any()
    grown = dt.grow_table(table, 1003, np.random.default_rng(1), zeros=True, fill=0.1)
    assert np.array_equal(grown[:1000], table) and (grown[1000:] == np.float32(0.1)).all() and grown.dtype == np.float32
    assert not dt.grow_table(table, 1003, np.random.default_rng(1), zeros=True)[1000:].any()


def test_shard_files_without_accumulators(tmp_path):
    base = str(tmp_path / "model.ckpt-5")
    _write(base, np.ones((100, 4), np.float32), 2, adagrad=False)           # an SGD checkpoint
    assert dt.shard_files(base, dt.slot_keys({"rel_embeddings": 0}, False, True))[1] == 100
    with pytest.raises(ValueError, match="has no adagrad"):                 # an Adagrad main file whose shard files lost them
        dt.shard_files(base, dt.slot_keys({"rel_embeddings/Adagrad": 0}, False, True))
    with pytest.raises(ValueError, match="has no adagrad"):
        dt.read_entity_rows(base, 0, 50, 4, "adagrad")
