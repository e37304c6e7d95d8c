"""opt_method "RowAdagrad" on the host: its spellings, the step plan of each model, the refusals, shared negatives, and the
per-row accumulators (`rowadagrad`, one float per entity row) in the shard files of a row-sharded checkpoint.  No GPU and no
engine library (tests/test_step_plan.py's and tests/test_adagrad_checkpoint_files.py's style; the device side is
tests/test_gpu_row_adagrad*.py)."""
import itertools

import numpy as np
import pytest

from openkeonspark_amd import KgeError, step_plan
from openkeonspark_amd import distribute_training as dt

TRANSE, TRANSH, TRANSR, TRANSD = 0, 1, 2, 3
NAMES = ("RowAdagrad", "rowadagrad", "row_adagrad")
BASE = dict(model_id=TRANSE, opt_method="RowAdagrad", sparse_rows=None, use_counts=True, counts_supported=1, ent_total=993, rel_total=7,
            width=64, batch_size=128, n_neg=1)


def plan(**kw):
    return step_plan.plan(**dict(BASE, **kw))


def flags(p):
    return ("c" if p.use_counts else "-") + ("r" if p.sparse_rows else "-") + ("i" if p.sparse_inplace else "-")


def test_spellings():
    for name in NAMES:
        assert step_plan.optimizer_kind(name) == "row_adagrad"
    for name in ("ROWADAGRAD", "Row_Adagrad", "RowAdaGrad", "rowAdagrad", "row-adagrad"):      # (no other spelling: SGD, as any unknown name)
        assert step_plan.optimizer_kind(name) == "sgd"
    assert step_plan.optimizer_kind("Adagrad") == "adagrad" and step_plan.optimizer_kind("LazyAdam") == "lazy_adam"


@pytest.mark.parametrize("name,wish", list(itertools.product(NAMES, (None, True, False))))
def test_the_plan_of_each_model(name, wish):
    """A small table, below every size rule: asking for the rule IS asking for touched rows, whatever `sparse_rows` says.  TransE
    on the sign-count path: sparse rows; off it, and TransH / TransD: in place from float records; TransR: dense tables."""
    p = plan(opt_method=name, sparse_rows=wish)
    assert flags(p) == "cr-"
    assert p.optimizer == "row_adagrad" and p.row_adagrad and p.rows_rule and not p.has_slots
    assert not (p.adam or p.lazy_adam or p.adagrad)
    assert flags(plan(opt_method=name, sparse_rows=wish, counts_supported=0)) == "--i"
    assert flags(plan(opt_method=name, sparse_rows=wish, use_counts=False)) == "--i"
    for mid in (TRANSH, TRANSD):
        p = plan(model_id=mid, opt_method=name, sparse_rows=wish, counts_supported=0)
        assert flags(p) == "--i" and p.row_adagrad and p.rows_rule and not p.has_slots
    if wish:
        with pytest.raises(KgeError, match="sparse_rows needs TransE / TransH / TransD"):
            plan(model_id=TRANSR, opt_method=name, sparse_rows=wish, counts_supported=0)
    else:
        p = plan(model_id=TRANSR, opt_method=name, sparse_rows=wish, counts_supported=0)
        assert flags(p) == "---" and p.row_adagrad and p.rows_rule and not p.has_slots


def test_the_other_kinds_are_not_row_adagrad():
    for name, kind in (("SGD", "sgd"), ("Adam", "adam"), ("LazyAdam", "lazy_adam"), ("Adagrad", "adagrad")):
        p = plan(opt_method=name)
        assert p.optimizer == kind and not p.row_adagrad
    assert plan(opt_method="Adagrad").rows_rule and not plan(opt_method="Adagrad").has_slots
    assert plan(opt_method="LazyAdam").rows_rule and plan(opt_method="LazyAdam").has_slots


def test_shards_at_creation_as_adagrad():
    p = plan()
    assert step_plan.shards_at_creation(p, TRANSE, 2, 64) and not step_plan.shards_at_creation(p, TRANSE, 1, 64)
    assert not step_plan.shards_at_creation(plan(model_id=TRANSH, counts_supported=0), TRANSH, 2, 64)


@pytest.mark.parametrize("acc0", [0, 0.0, -1, float("nan")])
def test_a_non_positive_initial_accumulator_is_refused_in_adagrads_words(acc0):
    for name in NAMES:
        with pytest.raises(KgeError) as err:
            plan(opt_method=name, adagrad_initial_accumulator=acc0)
        assert str(err.value) == ("adagrad_initial_accumulator must be positive (the Adagrad rule divides by sqrt(accumulator), without an "
                                  "epsilon), got %r" % (acc0,))
    assert not plan(opt_method="SGD", adagrad_initial_accumulator=acc0).row_adagrad         # (only the Adagrads read it)


def test_shared_negatives():
    """Accepted for TransE by position and by relation, and for TransH / TransD / TransR on relation-grouped chunks where the
    library says it has their kernels; the plans are the ones Adagrad gets."""
    for by_relation in (False, True):
        assert flags(plan(shared_chunk=8, by_relation=by_relation)) == "cr-"
    assert flags(plan(model_id=TRANSH, counts_supported=0, shared_chunk=8, by_relation=True, shared_float_supported=1)) == "--i"
    assert flags(plan(model_id=TRANSD, counts_supported=0, shared_chunk=8, by_relation=True, shared_transd_supported=1)) == "--i"
    p = plan(model_id=TRANSR, counts_supported=0, shared_chunk=8, by_relation=True, shared_transr_supported=1)
    assert flags(p) == "---" and p.row_adagrad
    for mid, flag in ((TRANSH, "shared_float_supported"), (TRANSD, "shared_transd_supported"), (TRANSR, "shared_transr_supported")):
        with pytest.raises(KgeError, match="built for TransE only"):            # without the flag: no kernel
            plan(model_id=mid, counts_supported=0, shared_chunk=8, by_relation=True)
        with pytest.raises(KgeError, match="by_relation=True"):                 # with it: relation-grouped chunks only
            plan(model_id=mid, counts_supported=0, shared_chunk=8, **{flag: 1})
    with pytest.raises(KgeError, match="sign-count path"):
        plan(counts_supported=0, shared_chunk=8)


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------

def _write(base, table, acc, world, rowadagrad=True):
    E = table.shape[0]
    chunk = -(-E // world)
    for g in range(world):
        lo, hi = min(g * chunk, E), min((g + 1) * chunk, E)
        extra = dict(rowadagrad=acc[lo:hi]) if rowadagrad else {}
        dt._atomic_savez(base + ".shard%dof%d.npz" % (g, world), rows=table[lo:hi], lo=np.int64(lo), hi=np.int64(hi),
                         ent_total=np.int64(E), **extra)


def test_which_arrays_a_resuming_run_reads():
    row_ckpt = {"rel_embeddings": 0, "rel_embeddings/RowAdagrad": 0, "global_step": 5}
    adagrad_ckpt = {"rel_embeddings": 0, "rel_embeddings/Adagrad": 0, "global_step": 5}
    adam_ckpt = {"rel_embeddings": 0, "rel_embeddings/Adam": 0, "rel_embeddings/Adam_1": 0, "beta1_power": 0.9, "beta2_power": 0.999}
    sgd_ckpt = {"rel_embeddings": 0, "global_step": 5}
    assert dt.slot_keys(row_ckpt, False, False, True) == ("rows", "rowadagrad")
    assert dt.slot_keys(row_ckpt, False, False, row_adagrad=True) == ("rows", "rowadagrad")
    for other in (sgd_ckpt, adam_ckpt, adagrad_ckpt):                       # resumed under RowAdagrad: fresh accumulators
        assert dt.slot_keys(other, False, False, True) == ("rows",)
    assert dt.slot_keys(row_ckpt, False, False) == ("rows",)                # a RowAdagrad checkpoint under SGD: ignored
    assert dt.slot_keys(row_ckpt, False, True) == ("rows",)                 # ... under Adagrad: fresh element accumulators
    assert dt.slot_keys(row_ckpt, True, False) == ("rows",)                 # ... under LazyAdam: zero moments
    assert dt.slot_keys(adagrad_ckpt, False, True) == ("rows", "adagrad")   # (the three-argument form as before)
    assert dt.slot_keys(adam_ckpt, True, False) == ("rows", "adam", "adam_1")


@pytest.mark.parametrize("world", [1, 2, 3])
def test_accumulator_rows_from_any_number_of_writers(tmp_path, world):
    rng = np.random.default_rng(world)
    table = rng.standard_normal((1001, 8)).astype(np.float32)
    acc = (0.1 + rng.random(1001)).astype(np.float32)
    base = str(tmp_path / "model.ckpt-7")
    _write(base, table, acc, world)
    parts = dt.shard_files(base, ("rows", "rowadagrad"))
    assert parts[1] == 1001
    for lo, hi in ((0, 1001), (333, 668), (1000, 1001)):
        got, ent_total = dt.read_entity_rows(base, lo, hi, None, "rowadagrad", parts, fill=0.1)
        assert ent_total == 1001 and got.shape == (hi - lo,) and got.dtype == np.float32 and np.array_equal(got, acc[lo:hi])
        rows, _ = dt.read_entity_rows(base, lo, hi, 8, "rows", parts)
        assert np.array_equal(rows, table[lo:hi])


def test_new_entities_get_the_initial_value(tmp_path):
    rng = np.random.default_rng(0)
    table, acc = rng.standard_normal((1000, 4)).astype(np.float32), (0.1 + rng.random(1000)).astype(np.float32)
    base = str(tmp_path / "model.ckpt-5")
    _write(base, table, acc, 2)
    got, ent_total = dt.read_entity_rows(base, 900, 1050, None, "rowadagrad", fill=0.25)      # a shard reaching past the checkpoint
    assert ent_total == 1000 and np.array_equal(got[:100], acc[900:]) and (got[100:] == np.float32(0.25)).all()
    got, _ = dt.read_entity_rows(base, 1050, 2100, None, "rowadagrad", fill=0.25)             # a shard of new entities only
    assert got.shape == (1050,) and (got == np.float32(0.25)).all()


def test_shard_files_without_accumulators(tmp_path):
    base = str(tmp_path / "model.ckpt-5")
    _write(base, np.ones((100, 4), np.float32), None, 2, rowadagrad=False)         # an SGD checkpoint
    assert dt.shard_files(base, dt.slot_keys({"rel_embeddings": 0}, False, False, True))[1] == 100
    with pytest.raises(ValueError, match="has no rowadagrad"):                     # a RowAdagrad main file whose shard files lost them
        dt.shard_files(base, dt.slot_keys({"rel_embeddings/RowAdagrad": 0}, False, False, True))
    with pytest.raises(ValueError, match="has no rowadagrad"):
        dt.read_entity_rows(base, 0, 50, None, "rowadagrad")


def test_the_driver_takes_the_name():
    args = dt.parse_args(["--optimizer", "RowAdagrad"])
    assert args.optimizer == "RowAdagrad" and step_plan.optimizer_kind(args.optimizer) == "row_adagrad"
