"""Which path a training step takes, decided once from plain values: no torch, no ctypes, no device.

`plan()` is what `Config.set_model_and_session` asks before it creates anything; `shards_at_creation()` what
`Config._plan_entity_shard` asks once it knows the world size; `large_counts_step()` the one predicate behind "TransE
sign-count step at a large batch" (the packed negatives, the prefetch default, the step itself, the persistent launch).
"""
from collections import namedtuple

from ._lib import KgeError, TRANSE, TRANSH, TRANSR, TRANSD

# accepted spellings of the optimizer names (distribute_training.py:95 for Adam); any other name trains with SGD, as the reference does
_KINDS = {"Adam": "adam", "adam": "adam",
          "LazyAdam": "lazy_adam", "lazyadam": "lazy_adam", "lazy_adam": "lazy_adam",
          "Adagrad": "adagrad", "adagrad": "adagrad",
          "RowAdagrad": "row_adagrad", "rowadagrad": "row_adagrad", "row_adagrad": "row_adagrad"}


def optimizer_kind(name):
    """"sgd", "adam", "lazy_adam", "adagrad" or "row_adagrad"."""
    return _KINDS.get(name, "sgd") if isinstance(name, str) else "sgd"


class StepPlan(namedtuple("StepPlan", "optimizer use_counts sparse_rows sparse_inplace table_bytes")):
    """optimizer: the kind (optimizer_kind).  use_counts: TransE's exact integer sign-count gradients instead of fp32 atomics.
    sparse_rows: the int8-record touched-rows step (one rank: sparse step; N ranks: the table-sharded step).  sparse_inplace:
    touched rows updated in place from float gradient records.  Neither: dense gradient tables (or the count image)."""
    __slots__ = ()

    @property
    def adam(self):
        return self.optimizer == "adam"

    @property
    def lazy_adam(self):
        return self.optimizer == "lazy_adam"

    @property
    def adagrad(self):
        return self.optimizer == "adagrad"

    @property
    def row_adagrad(self):
        return self.optimizer == "row_adagrad"

    @property
    def has_slots(self):
        """m / v tables and beta powers exist (both Adam flavours)."""
        return self.optimizer in ("adam", "lazy_adam")

    @property
    def rows_rule(self):
        """Optimizers that ARE a choice of touched rows."""
        return self.optimizer in ("lazy_adam", "adagrad", "row_adagrad")


def wants_sparse_rows(sparse_rows, ent_total, rel_total, width, batch_size, n_neg, sparse_threshold_bytes=None):
    """(table bytes, sparse rows wanted?) -- the caller's wish (`sparse_rows` True / False) or, left at None, the measured rule."""
    table_bytes = (ent_total + rel_total) * width * 4
    sparse = sparse_rows
    if sparse is None:
        # Measured cross-over on one MI355X (tools/sparse_crossover.sh, profiles/r03_sparse_crossover.jsonl: dim 512,
        # B = 131 072, n = 1, tables of 0.26 .. 8.2 GB): the dense step costs the batch's work plus a sweep of the whole
        # table and count image, the sparse step the batch's work plus its sort -- they tie at 0.26 GB (0.68 vs 0.70 ms),
        # sparse rows win by 18 % at 0.5 GB and 5.4x at 8 GB.  The tie sits where the table is ~0.3x the bytes of the rows
        # a step touches (1.07 GB there); below 128 MB the dense path's image fits the caches and it is kept.
        touched_bytes = batch_size * (3 + n_neg) * width * 4
        threshold = sparse_threshold_bytes
        if threshold is None:
            threshold = max(128 << 20, int(0.3 * touched_bytes))
        sparse = table_bytes > int(threshold)
    return table_bytes, sparse


def plan(model_id, opt_method, sparse_rows, use_counts, counts_supported, ent_total, rel_total, width, batch_size, n_neg,
         sparse_threshold_bytes=None, adagrad_initial_accumulator=0.1, shared_chunk=0, negative_rel=0, by_relation=False, typed=False,
         shared_float_supported=0, shared_transd_supported=0, shared_transr_supported=0, in_chunk=0, table_dtype="fp32",
         bf16_supported=0, bf16_shared_supported=0):
    """The StepPlan of a configuration.  sparse_rows: None = automatic, True / False = the caller's wish; use_counts: the
    caller's wish; counts_supported: what kge_transe_counts_supported said for the model's descriptor and n_neg.
    shared_chunk: 0 = off; P > 0 = negatives shared by chunks of P positives (NON-PARITY, opt-in: Config.set_shared_negatives),
    which is the sparse-rows record step whatever the table size; negative_rel: how many of the n_neg are relation negatives;
    by_relation: the chunks are cut from the batch ordered by relation (train_paths.shared_grouped_step); typed: type-constrained
    sampling is on, which shared negatives take on such chunks only; shared_float_supported: what kge_shared_float_supported said
    for the model's descriptor and the entity negatives (TransH on relation-grouped chunks, float gradient records);
    shared_transd_supported: what kge_shared_transd_supported said for them (TransD on such chunks, the same records with the
    transfer rows); shared_transr_supported: what kge_shared_transr_supported said for them (TransR on such chunks, through its
    dense gradient tables: the plan of its unshared step); in_chunk: K >= 0 of a chunk's candidates are its own positives' entities
    beside the n_neg - negative_rel drawn ones (relation-grouped chunks only); it is checked and changes no plan.
    table_dtype: "fp32", or "bf16" = the tables are STORED as bf16 (NON-PARITY, opt-in: Config.set_table_dtype), which is the
    sparse-rows record step whatever the table size, as for the rows-rule optimizers; bf16_supported: what kge_bf16_tables_supported
    said for the model's descriptor and n_neg; bf16_shared_supported: what kge_bf16_shared_supported said for the descriptor and the
    entity negatives with in_chunk -- the two modes together are the shared-negatives step on bf16 tables, one rank."""
    optimizer = optimizer_kind(opt_method)
    check_table_dtype(table_dtype)
    adam, lazy_adam, adagrad = optimizer == "adam", optimizer == "lazy_adam", optimizer == "adagrad"
    row_adagrad = optimizer == "row_adagrad"
    # LazyAdam -- opt-in, NON-PARITY: Adam on the touched rows only (tf.contrib.opt.LazyAdamOptimizer's rule) for tables whose dense
    # TF1-Adam sweep -- 32 bytes per element per step, the reference's semantics -- would dominate the step.
    # Adagrad -- opt-in: TF1's AdagradOptimizer (upstream OpenKE offers it; the reference sends the name to SGD).  Like LazyAdam it
    # rides on the touched-rows paths, but exactly: an element with zero gradient keeps its value and its accumulator bit for bit,
    # so "only the touched rows" IS the dense rule.  One accumulator table per parameter table, nothing to advance between steps.
    # TransR has no record path and keeps its dense gradient tables (kge_adagrad_update_tables), in one process only.
    # RowAdagrad -- opt-in: PyTorch-BigGraph's row-wise Adagrad, ONE accumulator per table row, which takes the mean squared gradient
    # of the row each step (a += sum g^2 / L; p -= lr * g / sqrt(a)).  Exact on the touched rows for Adagrad's reason -- a row whose
    # gradient is zero keeps its value and its accumulator bit for bit -- and on the same paths; it starts from the same positive
    # value (adagrad_initial_accumulator) and has no epsilon.  TransR: dense tables (kge_rowadagrad_update_tables), one process.
    if (adagrad or row_adagrad) and not (float(adagrad_initial_accumulator) > 0.0):
        raise KgeError("adagrad_initial_accumulator must be positive (the Adagrad rule divides by sqrt(accumulator), without an "
                       "epsilon), got %r" % (adagrad_initial_accumulator,))
    if table_dtype == "bf16":      # storage, not a shadow copy: the record step on the touched rows is the only step that reads it
        check_bf16_tables(model_id, optimizer, use_counts, counts_supported, width, shared_chunk, bf16_supported,
                          bf16_shared_supported, negative_rel)
        if shared_chunk:      # the chunk, the candidate counts, typed and in-chunk candidates: the shared step's own limits
            check_shared_negatives(model_id, optimizer, use_counts, shared_chunk, n_neg - negative_rel, negative_rel, by_relation, typed,
                                   in_chunk=in_chunk)
        return StepPlan(optimizer, True, True, False, (ent_total + rel_total) * width * 2)
    rows_rule = lazy_adam or adagrad or row_adagrad
    # TransE: exact integer sign-count gradients instead of fp32 atomics (include/kge_mi355.h)
    use_counts = bool(use_counts) and bool(counts_supported)
    # sparse-row mode: no dense gradient / count image at all.  The int8 records are reduced into a compact
    # [touched rows, D] image and only those rows are updated; across ranks the records themselves are
    # all-gathered (the sparse touched-row exchange of BASELINE config #5).  Not with Adam: TF1's sparse Adam
    # sweeps every row of m, v and the table each step, which is the dense path by definition.
    table_bytes, sparse = wants_sparse_rows(sparse_rows, ent_total, rel_total, width, batch_size, n_neg, sparse_threshold_bytes)
    rows = (bool(sparse) or rows_rule) and use_counts and not adam
    if shared_chunk:
        check_shared_negatives(model_id, optimizer, use_counts, shared_chunk, n_neg - negative_rel, negative_rel, by_relation, typed,
                               shared_float_supported, shared_transd_supported, shared_transr_supported, in_chunk)
        if model_id == TRANSR:      # dense gradient tables and the optimizer on the whole tables, as its unshared step
            return StepPlan(optimizer, False, False, False, table_bytes)
        if model_id in (TRANSH, TRANSD):      # float records, keyed in the unshared step's row space: the touched-rows plan in place
            return StepPlan(optimizer, False, False, True, table_bytes)
        return StepPlan(optimizer, use_counts, True, False, table_bytes)      # its records go through the touched-rows reduce
    # TransH / TransD (and TransE outside the sign-count path) with SGD: the touched rows are updated in place from float
    # gradient records (kge_forward_backward_sgd_rows) -- no gradient tables, no sweep.  On request, or by itself for tables
    # beyond 2 GB (measured at 4 GB, dim 200, B = 131 072, n = 1: TransH 1.63 -> 0.70 ms, TransD 2.83 -> 0.97 ms per step and
    # half the memory, profiles/r03_h_*; the dense form's sweep scales with the table, so the two tie near 1 GB)
    # With LazyAdam the same records end in the Adam rule on the touched rows and their moments instead of the add
    # (kge_forward_backward_adam_rows): asking for LazyAdam IS asking for touched rows, whatever `sparse_rows` says.
    vector_model = model_id in (TRANSE, TRANSH, TRANSD)
    inplace = bool(not rows and vector_model and not adam and
                   (rows_rule or sparse_rows or (sparse_rows is None and table_bytes > (2 << 30))))
    if lazy_adam and not (rows or inplace):
        raise KgeError("LazyAdam (touched rows only, NON-PARITY) needs TransE, TransH or TransD: TransR's gradient is a whole "
                       "matrix per relation and has no record path")
    if sparse_rows and not (rows or inplace):
        raise KgeError("sparse_rows needs TransE / TransH / TransD with SGD, LazyAdam or Adagrad")
    return StepPlan(optimizer, use_counts, rows, inplace, table_bytes)


TABLE_DTYPES = ("fp32", "bf16")


def check_table_dtype(table_dtype):
    if table_dtype not in TABLE_DTYPES:
        raise KgeError("table_dtype is \"fp32\" or \"bf16\", got %r" % (table_dtype,))


BF16_SHARED_MAX_WIDTH = 512      # the shared emit kernel's LDS tiles


def check_bf16_tables(model_id, optimizer, use_counts, counts_supported, width, shared_chunk=0, bf16_supported=1, bf16_shared_supported=0,
                      negative_rel=0):
    """Raises KgeError, naming the limit, for a configuration that bf16 table storage cannot take: it is built for TransE on the
    one-rank int8-record touched-rows step with SGD or RowAdagrad (include/kge_mi355.h, "bf16 table storage").  shared_chunk > 0:
    together with shared negatives, which the shared emit kernel takes on bf16 tables where kge_bf16_shared_supported says so
    (bf16_shared_supported: its answer; "Shared negatives on bf16 tables")."""
    if model_id != TRANSE:
        raise KgeError("bf16 table storage is built for TransE only: TransH, TransD and TransR have no bf16 emit kernel"
                       + (", shared or not: their tables stay fp32" if shared_chunk else ""))
    if shared_chunk and negative_rel:
        raise KgeError("bf16 table storage with shared negatives: relation negatives are not supported (negative_rel must be 0, "
                       "got %d)" % negative_rel)
    if shared_chunk and width > BF16_SHARED_MAX_WIDTH:
        raise KgeError("bf16 table storage with shared negatives: the shared emit kernel holds embedding widths up to %d, got %d"
                       % (BF16_SHARED_MAX_WIDTH, width))
    if optimizer not in ("sgd", "row_adagrad"):
        raise KgeError("bf16 table storage needs SGD or RowAdagrad: LazyAdam, Adagrad and TF1 Adam keep fp32 slot tables shaped like "
                       "the parameter tables and have no bf16 apply kernel")
    if width % 8 != 0:
        raise KgeError("bf16 table storage needs an embedding width that is a multiple of 8 (rows of 16-byte chunks), got %d" % width)
    if not (use_counts and counts_supported):
        raise KgeError("bf16 table storage needs TransE's sign-count path (use_counts, and a shape kge_transe_counts_supported "
                       "accepts: width up to 1024, 1 to 63 negatives)")
    if not bf16_supported:
        raise KgeError("bf16 table storage: kge_bf16_tables_supported refuses this shape (TransE, width a multiple of 8 up to 1024)")
    if shared_chunk and not bf16_shared_supported:
        raise KgeError("bf16 table storage cannot be combined with shared negatives at this shape: kge_bf16_shared_supported refuses "
                       "it (TransE, entity negatives only, a width that is a multiple of 8 up to %d, 1 to %d candidates per "
                       "positive)" % (BF16_SHARED_MAX_WIDTH, SHARED_MAX_NEGATIVES))


def check_bf16_shared_seeds(table_seed, shared_seed):
    """Raises KgeError when bf16 table storage and shared negatives would hash from the same seed.  Both counter hashes start from
    the step key mix(seed + (step + 1) G) (include/kge_mi355.h: "Stochastic rounding", "Candidates"): with equal seeds the 64 bits
    that round the columns 4 g .. 4 g + 3 of row `key` are the bits that drew the candidate or the side whose counter equals
    key (D / 4) + g, and the rounding would no longer be independent of the rows a step updates.  The definitions of the two
    hashes are fixed (runs repeat bit for bit), so the seeds must differ."""
    if int(table_seed) == int(shared_seed):
        raise KgeError("bf16 table storage with shared negatives: the rounding seed and the shared-negatives seed must differ (both are "
                       "%d): the two counter hashes share their step key, so with one seed the bits that round a row are the bits that "
                       "drew a candidate -- set_table_dtype(\"bf16\", seed=...) / set_shared_negatives(chunk, seed=...), "
                       "--table_rounding_seed / --shared_negatives_seed" % int(table_seed))


SHARED_MAX_CHUNK, SHARED_MAX_NEGATIVES = 127, 63      # a candidate's count lies within +-P, a positive's within +-2N: both int8


TYPED_NEEDS_BY_RELATION = ("a chunk of consecutive batch positions mixes relations, so its candidates cannot come from one relation's "
                           "type list; set_shared_negatives(chunk, by_relation=True) orders the batch by relation and draws typed "
                           "candidates (without by_relation typed candidates are not built)")


def check_in_chunk(in_chunk, by_relation):
    """Raises KgeError for an in-chunk candidate count that is negative, or positive without relation-grouped chunks."""
    if int(in_chunk) < 0:
        raise KgeError("shared negatives: in_chunk counts the candidates a chunk takes from its own positives and must be 0 or more, "
                       "got %r" % (in_chunk,))
    if in_chunk and not by_relation:
        raise KgeError("shared negatives: in-chunk candidates need chunks of one relation -- set_shared_negatives(chunk, "
                       "by_relation=True, in_chunk=%d): in a chunk by position a candidate has no single side, and on more than one "
                       "rank a slice of another rank would own its entities" % in_chunk)


def check_shared_negatives(model_id, optimizer, use_counts, chunk, negative_ent, negative_rel, by_relation=False, typed=False,
                           shared_float_supported=0, shared_transd_supported=0, shared_transr_supported=0, in_chunk=0):
    """Raises KgeError, naming the limit, for a configuration the shared-negatives step cannot take.  by_relation: chunks cut from
    the batch ordered by relation; typed: candidates from the relations' type lists, which needs by_relation;
    shared_float_supported: the library's answer for TransH on such chunks (kge_shared_float_supported), which needs no use_counts;
    shared_transd_supported: its answer for TransD on them (kge_shared_transd_supported), likewise; shared_transr_supported: its
    answer for TransR on them (kge_shared_transr_supported): dense gradient tables, so TF1 Adam is taken and LazyAdam is not.
    in_chunk: K of a chunk's candidates are the entities of its own positives (include/kge_mi355.h, "In-chunk candidates"), beside the
    negative_ent drawn ones."""
    if typed and not by_relation:
        raise KgeError("shared negatives cannot be combined with type-constrained sampling: " + TYPED_NEEDS_BY_RELATION)
    if not 1 <= int(chunk) <= SHARED_MAX_CHUNK:
        raise KgeError("shared negatives: a chunk holds 1 to %d positives (a candidate's count lies within +-chunk and is carried "
                       "as an int8), got %r" % (SHARED_MAX_CHUNK, chunk))
    check_in_chunk(in_chunk, by_relation)
    transh =model_id == TRANSH and bool(shared_float_supported)
    if transh and not by_relation:
        raise KgeError("shared negatives on chunks by position are built for TransE only: TransH shares one normal vector per chunk, "
                       "which needs chunks of one relation -- set_shared_negatives(chunk, by_relation=True)")
    transd = model_id == TRANSD and bool(shared_transd_supported)
    if transd and not by_relation:
        raise KgeError("shared negatives on chunks by position are built for TransE only: TransD shares one transfer vector per chunk, "
                       "which needs chunks of one relation -- set_shared_negatives(chunk, by_relation=True)")
    transr = model_id == TRANSR and bool(shared_transr_supported)
    if transr and not by_relation:
        raise KgeError("shared negatives on chunks by position are built for TransE only: TransR shares one matrix per chunk, "
                       "which needs chunks of one relation -- set_shared_negatives(chunk, by_relation=True)")
    if model_id != TRANSE and not transh and not transd and not transr:
        raise KgeError("shared negatives are built for TransE only: TransH, TransD and TransR have no shared emit kernel")
    if negative_rel > 0:
        raise KgeError("shared negatives: relation negatives are not supported (negative_rel must be 0, got %d)" % negative_rel)
    if not 1 <= negative_ent <= SHARED_MAX_NEGATIVES:
        raise KgeError("shared negatives: 1 to %d negatives per positive (a positive's count lies within +-2N and is carried as "
                       "an int8), got %d" % (SHARED_MAX_NEGATIVES, negative_ent))
    if negative_ent + int(in_chunk) > SHARED_MAX_NEGATIVES:
        raise KgeError("shared negatives: drawn and in-chunk candidates together are at most %d per positive (a positive's count lies "
                       "within +-2 (N + in_chunk) and is carried as an int8), got %d + %d"
                       % (SHARED_MAX_NEGATIVES, negative_ent, in_chunk))
    if transr:      # (the gradients are dense tables: SGD, Adagrad, RowAdagrad and TF1 Adam sweep them as they do in the unshared step)
        if optimizer == "lazy_adam":
            raise KgeError("LazyAdam (touched rows only, NON-PARITY) needs TransE, TransH or TransD: TransR's gradient is a whole "
                           "matrix per relation and has no record path")
        return
    if optimizer == "adam":
        raise KgeError("shared negatives need SGD, LazyAdam or Adagrad: with TF1 Adam the dense count image has no entrance for "
                       "shared records yet")
    if not use_counts and not transh and not transd:
        raise KgeError("shared negatives need TransE's sign-count path (use_counts, and a shape kge_transe_counts_supported accepts)")


def shards_at_creation(step_plan, model_id, world, width):
    """Does a world of `world` ranks create the entity table row-sharded?  Where the step will be the table-sharded sparse one:
    TransE on the sign-count path with SGD, LazyAdam or Adagrad, 2 to 64 ranks, a width that is a multiple of 4."""
    return bool(1 < world <= 64 and width % 4 == 0 and model_id == TRANSE and step_plan.sparse_rows)


def large_counts_step(step_plan, n_pos, n_neg, counts_min_records, world):
    """TransE sign-count step at a large batch?  Steps with fewer gradient rows than counts_min_records per rank take the single
    fused fp32-atomic kernel instead (launch-bound regime, tools/sweep_paths.py).  The same decision on every rank: it depends
    on the global batch only."""
    return (step_plan.use_counts and not step_plan.sparse_rows and not step_plan.sparse_inplace and
            n_pos * (3 + n_neg) >= counts_min_records * world)      # (called once per training step: kept to one expression)
