"""`Config`: the reference's binding / hyper-parameter / session object (/root/reference/Config.py)
re-hosted on the MI355X engine.

Same constructor, setters, attributes, `init()` and `sampling()` as the reference
(Config.py:17-72,153-210,225-347), so `distribute_training.get_conf`-style callers work unchanged
(distribute_training.py:32-71).  What the reference did with a TensorFlow session --
`sess.run([train_op, loss, global_step], feed_dict)` (distribute_training.py:282) built by
`create_model` (distribute_training.py:74-105) -- is `train_step()` here: sample on the device,
run the fused forward/backward operator, exchange gradients over RCCL when data-parallel, apply
SGD, TF-parity Adam or -- opt-in -- lazy Adam / Adagrad / row-wise Adagrad on the touched rows.  Nothing in this module computes on the CPU; without the HIP library or a
GPU the device calls raise.
"""
import ctypes
import json
import os
import sys

import numpy as np

from . import _lib, rank_eval, shard_eval, step_plan, train_paths
from ._lib import KgeError


class Config(object):
    '''
    use ctypes to call the engine's C ABI from python and set essential parameters.
    '''

    def __init__(self, cpp_lib_path=None, init_new_entities=False):
        self.init_new_entities = init_new_entities
        if init_new_entities == False:
            # C library (Config.py:28-31): defaults to the in-tree MI355X engine
            if cpp_lib_path is None:
                cpp_lib_path = _lib.LIB_PATH
            self.lib = _lib.load(os.path.abspath(cpp_lib_path))
            # other parameters (Config.py:53-72)
            self.in_path = None
            self.out_path = None
            self.bern = 0
            self.hidden_size = 64
            self.ent_size = self.hidden_size
            self.rel_size = self.hidden_size
            self.train_times = 0
            self.margin = 1.0
            self.nbatches = 0
            self.negative_ent = 1
            self.negative_rel = 0
            self.workThreads = 8
            self.alpha = 0.001
            self.exportName = None
            self.importName = None
            self.opt_method = "SGD"
            self.test_link_prediction = False
            self.test_relation_prediction = False
            self.test_triple_classification = False
            self.valid_triple_classification = False
            self.type_constrained_sampling = False
            self._shared_chunk, self._shared_seed = 0, 0      # set_shared_negatives
            self._shared_by_relation = False                  # ... its chunks are cut from the batch ordered by relation
            self._shared_in_chunk = 0                         # ... K of a chunk's candidates are its own positives' entities
            self._table_dtype, self._table_seed = "fp32", 0   # set_table_dtype
            self._eval_view = None                            # bf16 tables: the float32 view the full-entity evaluators read (_tab_ptrs)
            self._bf16_evaluation = "view"                    # set_bf16_evaluation
            # engine-side additions
            self.seed = 0                 # parameter initialisation seed
            self.device = "cuda"
            self.adam_beta1, self.adam_beta2, self.adam_epsilon = 0.9, 0.999, 1e-8  # TF1 AdamOptimizer defaults
            self.adagrad_initial_accumulator = 0.1   # TF1 AdagradOptimizer's default; must be positive (the rule has no epsilon)
            self._adagrad = False                    # set_model_and_session decides it from opt_method
            self._row_adagrad = False                # likewise ("RowAdagrad": one accumulator per table row, from the same initial value)
            self.trainModel = None
            self.global_step = 0
            self.rank, self.world_size = 0, 1
            self._pg = None
            # link_prediction and relation_prediction on an entity table sharded across ranks: the test set goes in chunks
            # whose fetched query rows (2 rows of 4 * dim bytes per triple) take at most this many bytes (at least one triple
            # per chunk; for relation_prediction, the smallest value over the ranks holds)
            self.lp_shard_query_bytes = 256 << 20
            # top_k_tails / top_k_heads on such a table: all ranks' queries go in chunks whose fetched fixed-side rows and key
            # lists (4 * dim + 8 * k bytes per query) take at most this many bytes (at least one query per chunk; the smallest
            # value over the ranks holds)
            self.topk_shard_query_bytes = 256 << 20

    # ------------------------------------------------------------------------------------------
    # Config.py:153-210
    # ------------------------------------------------------------------------------------------
    def init(self):
        '''
        prepare for train and test
        '''
        if self.init_new_entities == False:
            self.trainModel = None
            self._forget_evaluation()
            if self.in_path != None:
                path = self.in_path if self.in_path.endswith("/") else self.in_path + "/"
                self.lib.kge_clear_error()
                self.lib.setInPath(path.encode())
                self.lib.setBern(self.bern)
                self.lib.setWorkThreads(self.workThreads)
                self.lib.randReset()
                self.lib.importTrainFiles()
                _lib.raise_if_error(self.lib)
                self.relTotal = self.lib.getRelationTotal()
                self.entTotal = self.lib.getEntityTotal()
                self.trainTotal = self.lib.getTrainTotal_()
                self.testTotal = self.lib.getTestTotal()
                self.validTotal = self.lib.getValidTotal()
                self.bt = self.lib.getBatchTotal()
                self.set_mini_batch()
                self._alloc_batch_buffers()
            if self.test_link_prediction or self.test_relation_prediction:
                self.init_link_prediction()
            if self.in_path != None:
                self._apply_typed_sampling()      # (the engine is one per process: an earlier Config's setting must not linger)
            # triple-classification inputs (Test.h:266-444) are not built yet

    def init_link_prediction(self):
        r'''
        import essential files for link prediction (Config.py:74-80); type / ontology constraints are
        optional here (the reference crashes without them)
        '''
        path = self.in_path if self.in_path.endswith("/") else self.in_path + "/"
        derived = getattr(self, "_type_lists_from", None) == "derived"
        self.lib.kge_clear_error()
        self.lib.importTestFiles()
        self._forget_evaluation()
        if derived:      # the lists were derived from the triples (derive_type_constraints), not read: derive them from this import too
            self.derive_type_constraints()
        elif os.path.exists(path + "type_constrain.txt"):
            self.lib.importTypeFiles()
        if os.path.exists(path + "ontology_constrain.txt"):
            self.lib.importOntologyFiles()
        _lib.raise_if_error(self.lib)
        self.testTotal = self.lib.getTestTotal()
        self.validTotal = self.lib.getValidTotal()
        if self.type_constrained_sampling:        # importTestFiles dropped the type lists: typed sampling needs them (and says so if they are gone)
            self._apply_typed_sampling()

    def set_type_constrained_sampling(self, flag):
        """Type-constrained negative sampling (NON-PARITY, off by default): an entity negative is drawn from the corrupted side's
        type list of its relation (type_constrain.txt) minus the known triples, instead of from all entities; a relation without
        a list, or a group that exhausts its list, falls back to the untyped draw.  Same random stream, positives, head-or-tail
        coins and relation negatives (include/kge_mi355.h kge_set_typed_sampling has the exact draw).  Callable before init(),
        which then imports type_constrain.txt even when link prediction is off, or after it, for the batches drawn from then
        on.  While it is on the sampler is a launch of its own and persistent_supported() is False.  The lists need not come
        from the file: after init_evaluation_from_arrays(..., type_lists=...) / (..., derive_types=True) or
        derive_type_constraints() the engine's lists are used as they stand, which is how a graph given by init_from_arrays
        gets typed negatives."""
        if flag and self._shared_chunk and not self._shared_by_relation:
            raise KgeError("type-constrained sampling cannot be combined with shared negatives: " + step_plan.TYPED_NEEDS_BY_RELATION)
        self.type_constrained_sampling = bool(flag)
        if getattr(self, "trainTotal", None) is not None:      # after init(): switch the engine now
            self._apply_typed_sampling()

    def set_shared_negatives(self, chunk, seed=0, by_relation=False, in_chunk=0):
        """Negatives SHARED by chunks of positives (NON-PARITY, opt-in, off by default; the reference draws every negative for
        one positive): `chunk` consecutive positives of a batch score the same set_ent_neg_rate(N) candidate entities, drawn
        from a counter hash of (seed, global_step) -- what PyTorch-BigGraph and DGL-KE do -- so a chunk gathers 3 chunk + N table
        rows instead of chunk (3 + N).  A pair whose corrupted triple is a training triple is masked: it adds nothing to the loss
        and stays in its denominator (include/kge_mi355.h has the exact definition).  TransE on the sign-count path with SGD,
        LazyAdam or Adagrad, entity negatives only, 1 <= chunk <= 127, N <= 63; on more than one rank the entity table is
        row-sharded (a width that is a multiple of 4, up to 64 ranks) and a chunk's rows cross the wire once per chunk, not once
        per pair; the run equals the one-process run bit for bit at any rank count.  Call it before
        set_model_and_session; chunk = 0 switches it off.  In this mode prefetch_sampling is ignored (the positives are drawn
        when the step starts), hand-fed batches are refused and there is no persistent launch.
        by_relation=True: the step's positives are ordered by relation (stable) and a chunk never crosses a relation boundary --
        the run of a relation is cut into pieces of `chunk`, the last may be short (train_paths.shared_grouped_step; the
        definition is in include/kge_mi355.h).  A candidate then has ONE side for its whole chunk, and with
        set_type_constrained_sampling(True), in either call order, it is drawn from that side's type list of the chunk's relation
        (all entities for a relation without a list); the lists are found as typed sampling finds them.  One rank only: a
        rank's slice would need the order of the whole batch.
        TransH trains on shared negatives with by_relation=True only (widths up to 512; SGD, LazyAdam or Adagrad): a chunk of one
        relation also shares the normalised normal vector and r^, and a candidate is projected once per chunk; its float
        gradient records go through the touched-rows rule of the unshared TransH step (include/kge_mi355.h, "TransH on
        relation-grouped chunks").  TransD trains the same way (by_relation=True only, widths up to 512, the same three
        optimizers): a chunk shares r^ and its relation's raw transfer vector, an entity's two rows are gathered once per chunk, and
        every entity writes two float records, one for its ent_embeddings row and one for its ent_transfer row ("TransD on
        relation-grouped chunks").  TransR trains the same way (by_relation=True only, rel_dim up to 512; SGD, Adagrad or TF1 Adam,
        not LazyAdam): a chunk shares its relation's matrix, so 2 chunk + N rows go through the projection, dgrad and wgrad GEMMs
        where the unshared step puts chunk (2 + N), and the gradients are the dense tables of the unshared TransR step ("TransR on
        relation-grouped chunks").
        in_chunk=K (by_relation=True only, every model above): beside the N drawn candidates a chunk scores K of its OWN entities --
        PyTorch-BigGraph's batch negatives: column N + i of a chunk is the tail (the head, for a new-head column) of the positive
        at rotated position i of the chunk, so the K candidates follow the data distribution and are observed heads / tails of
        the chunk's relation whether or not it has a type list, which is not consulted for them.  A chunk shorter than K leaves
        the columns past its length empty (-1, masked); a candidate equal to the entity it would replace is masked.  The loss and
        every record count take N + K where they took N; N + K <= 63 ("In-chunk candidates").  0 = off: the step is today's."""
        if self.trainModel is not None:
            raise KgeError("set_shared_negatives must be called before set_model_and_session: it decides the step's path")
        chunk = int(chunk)
        if chunk and not 1 <= chunk <= step_plan.SHARED_MAX_CHUNK:
            raise KgeError("shared negatives: a chunk holds 1 to %d positives (a candidate's count lies within +-chunk and is "
                           "carried as an int8), got %d" % (step_plan.SHARED_MAX_CHUNK, chunk))
        by_relation = bool(by_relation) and chunk > 0
        if chunk and self.type_constrained_sampling and not by_relation:
            raise KgeError("shared negatives cannot be combined with type-constrained sampling: " + step_plan.TYPED_NEEDS_BY_RELATION)
        in_chunk = int(in_chunk) if chunk else 0
        step_plan.check_in_chunk(in_chunk, by_relation)
        self._shared_chunk, self._shared_seed, self._shared_by_relation = chunk, int(seed) & 0xFFFFFFFFFFFFFFFF, by_relation
        self._shared_in_chunk = in_chunk

    def set_table_dtype(self, dtype, seed=0):
        """How TransE's tables are STORED (before set_model_and_session).  "fp32": the default.  "bf16" (NON-PARITY, opt-in;
        the definition is in include/kge_mi355.h, "bf16 table storage"): ent_embeddings and rel_embeddings are bf16 tensors -- half
        the bytes in memory and in every gather and touched-row update -- trained on the one-rank int8-record touched-rows step
        with SGD or RowAdagrad; every updated row is stored by stochastic rounding from a hash of (seed, global step, row,
        column), so a run is reproducible bit for bit and a resumed run must repeat the seed.  get_parameters / checkpoints give
        float32 (an exact widening), set_parameters rounds to nearest-even.  test_step, triple classification, rank_candidates,
        rank_triples_sampled and validation_link_prediction(candidates=C) read the stored bf16 rows directly, with the same score
        bits and counts and no view.  The full-entity evaluators read a float32 view that lives until the next training step;
        rank_triples, validation_link_prediction(), top_k_tails and top_k_heads can instead stream the stored rows, with the same
        counts, ids and score bits and no memory of the table's size (set_bf16_evaluation("stored")), and do so by themselves when
        the view cannot be allocated.  link_prediction, relation_prediction and top_k_relations have no stored form and need
        the view.  Configurations the mode cannot take are refused by set_model_and_session.
        With set_shared_negatives(chunk, ...), in either call order, the shared step reads the bf16 tables (one rank, widths up to
        512, chunks by position or by relation, typed and in-chunk candidates included): its records are the fp32 shared emit's
        on the widened tables bit for bit (include/kge_mi355.h, "Shared negatives on bf16 tables").  The two seeds must then
        differ -- both hashes start from the same step key, so one seed would round rows with the bits that drew the candidates --
        and set_model_and_session refuses equal ones, the two defaults of 0 included."""
        step_plan.check_table_dtype(dtype)
        seed = int(seed)
        if not 0 <= seed < (1 << 64):
            raise KgeError("set_table_dtype: the rounding seed is an unsigned 64-bit value, got %r" % (seed,))
        self._table_dtype, self._table_seed = dtype, seed

    def set_bf16_evaluation(self, mode):
        """What rank_triples, validation_link_prediction() without candidates (the driver's early stop on hits10 / mrr included),
        top_k_tails and top_k_heads read on bf16 tables (set_table_dtype); no effect on fp32 tables, and it may be called at any
        time.  "view" (the default): the float32 view of the tables, made once and cached until the next training step -- twice
        the tables' bytes again, and kge_rank_triples builds an [E, D] float32 candidate table beside it; the faster choice where
        it fits.  When the view cannot be allocated these methods read the stored rows instead and say so on stderr.  "stored":
        kge_rank_triples_bf16 / kge_topk_entities_bf16 (include/kge_mi355.h, "Evaluation on bf16 tables") stream the stored bf16
        rows: the same counts, ids and score bits, nothing allocated that grows with E * D, and no view is made or dropped."""
        if mode not in ("view", "stored"):
            raise KgeError("set_bf16_evaluation: mode must be \"view\" or \"stored\", got %r" % (mode,))
        self._bf16_evaluation = mode

    @property
    def _bf16(self):
        return getattr(self, "_table_dtype", "fp32") == "bf16"

    def _refuse_bf16_ranks(self):
        """bf16 table storage is one rank: the row-sharded step and the replicated exchanges move fp32 rows."""
        if self._bf16 and self._dp:
            raise KgeError("bf16 table storage is single-process only: the row-sharded step and the data-parallel exchanges are "
                           "built for fp32 tables (world size %d)" % self.world_size)

    # The full-entity evaluation kernels read fp32 tables.  With bf16 storage every path that passes `_tab_ptrs` gets a float32 view
    # made by widening (exact), cached until the next training step or set_parameters and freed there: training memory is
    # unaffected.  The evaluators that only gather rows (_predict, rank_eval.rank_candidates_device) take _bf16_eval_tables instead.
    @property
    def _tab_ptrs(self):
        if self._bf16 and getattr(self, "_tables", None):
            return self._eval_table_ptrs()
        return self._tab_ptrs_raw

    @_tab_ptrs.setter
    def _tab_ptrs(self, value):
        self._tab_ptrs_raw = value

    def _eval_table_ptrs(self):
        import torch
        if self._eval_view is None:
            need = sum(t.numel() for t in self._tables) * 4
            try:
                views = [t.float() for t in self._tables]
            except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
                raise self._eval_view_error(need, str(e).splitlines()[0] if str(e) else type(e).__name__)
            self._eval_view = (views, _lib.table_ptrs([v.data_ptr() for v in views]))
        return self._eval_view[1]

    @staticmethod
    def _eval_view_error(need, why):
        return KgeError("bf16 table storage: link_prediction, relation_prediction and top_k_relations read a float32 view of the "
                        "tables and its %d bytes could not be allocated (%s).  rank_triples, validation_link_prediction(), "
                        "top_k_tails and top_k_heads rank and select over every entity from the stored bf16 rows and need no view; "
                        "so do test_step, triple_classification, validation_accuracy, roc_auc, rank_candidates, "
                        "rank_triples_sampled and validation_link_prediction(candidates=C)" % (need, why))

    def _bf16_full_eval_tables(self, what):
        """The stored bf16 tables' addresses (ent, rel) when the full-entity evaluator `what` (rank_eval.rank_device,
        rank_eval.top_k_entities) is to stream the stored rows (kge_rank_triples_bf16 / kge_topk_entities_bf16), else None: fp32
        tables, or "view" mode with a view that exists or can be made.  "stored" mode makes no view and drops none."""
        raw = self._bf16_eval_tables()
        if raw is None or self._bf16_evaluation == "stored":
            return raw
        try:
            self._eval_table_ptrs()
        except KgeError:
            print("%s: the float32 view of the bf16 tables could not be allocated; reading the stored bf16 rows instead "
                  "(the same results)" % what, file=sys.stderr)
            return raw
        return None

    def _drop_eval_view(self):
        self._eval_view = None

    def _bf16_eval_tables(self):
        """The stored bf16 tables' addresses (ent, rel) where the evaluators that gather rows read them directly
        (kge_predict_bf16, kge_rank_candidates_bf16; include/kge_mi355.h, "Evaluation on bf16 tables"), else None.  Asking
        makes no float32 view."""
        if not (self._bf16 and getattr(self, "_tables", None)):
            return None
        if not self.lib.kge_bf16_eval_supported(ctypes.byref(self._desc)):
            return None
        return self._tables[0].data_ptr(), self._tables[1].data_ptr()

    def _predict(self, h_ptr, t_ptr, r_ptr, n, out_ptr):
        """kge_predict on the tables as they are stored: bf16 tables are scored from their own rows, with the same bits."""
        raw = self._bf16_eval_tables()
        if raw is not None:
            rc = self.lib.kge_predict_bf16(ctypes.byref(self._desc), raw[0], raw[1], h_ptr, t_ptr, r_ptr, n, out_ptr, self._stream())
        else:
            rc = self.lib.kge_predict(ctypes.byref(self._desc), self._tab_ptrs, h_ptr, t_ptr, r_ptr, n, out_ptr, self._stream())
        _lib.check(rc, self.lib)

    def _refuse_shared_ranks(self, stepping=False):
        """Shared negatives across ranks train a row-sharded entity table (train_paths.shared_sharded_step) and nothing else:
        refuse, naming the limit, a world whose table cannot be sharded by rows and -- `stepping`: a step is about to run -- a
        data-parallel step without the shards."""
        if not (self._shared_chunk and self._dp):
            return
        if self._shared_by_relation:
            raise KgeError("shared negatives by relation train on one rank only: the chunks are cut from the whole batch ordered by "
                           "relation, and a rank's slice of the batch would need that global order (this run: %d ranks)"
                           % self.world_size)
        if self.hidden_size % 4 or self.world_size > 64:
            raise KgeError("shared negatives on more than one rank train a row-sharded entity table, which needs an embedding "
                           "width that is a multiple of 4 (this run: %d) and at most 64 ranks (this run: %d); there is no "
                           "replicated-table step for shared records" % (self.hidden_size, self.world_size))
        if stepping and not hasattr(self, "_shard"):
            raise KgeError("shared negatives: a data-parallel step needs the row shards that init_distributed() lays out "
                           "(force_data_parallel alone sets none up); without them shared negatives train on one rank only")

    def shared_negatives_of(self, step):
        """(cand int32 [n_chunks, N], pair uint8 [n_pos, N]) of the batch that training step `step` (its global_step when it
        began) trained on: the candidate ids of every chunk, and per (positive, candidate) bit 0 = side (0 new tail, 1 new head),
        bit 1 = masked.  On more than one rank these are the rank's OWN lists: its slice holds the batch positions
        [_first_pos, _first_pos + n_pos), row 0 of `pair` is position _first_pos and row 0 of `cand` is global chunk
        _first_pos // chunk -- which the rank may share with its neighbour, each holding the same candidates for it.
        An inspector: the lists of the most recent step are kept, no others (a pair's mask depends on the step's
        positives, which are not).
        With by_relation=True: (cand [n_chunks, N], pair [n_pos, N], perm int32 [n_pos], chunks int32 [n_chunks, 2]) -- row b of
        `pair` is SORTED position b, which holds batch position perm[b]; chunks[j] = (first sorted position, length) of chunk j,
        whose candidates are row j of `cand`; bit 0 of pair[b][k] is the side of candidate k, the same for every b of a chunk.
        With in_chunk=K the lists are N + K wide: columns 0 .. N - 1 are the drawn candidates, the same ids and sides as with
        K = 0; columns N .. N + K - 1 are the chunk's own entities (train_paths.shared_in_chunk_candidates), -1 past its length."""
        buf = self._sparse_buf if self._shared_chunk else None
        if not buf or buf.get("shared_step") != int(step):
            raise KgeError("shared_negatives_of: only the lists of the most recent shared-negatives step are kept (step %s)"
                           % (buf.get("shared_step") if buf else None))
        n_pos, n_chunks = buf["shared_shape"]
        if self._shared_by_relation:      # (cand[:n_chunks], pair by SORTED position, perm, chunks[:n_chunks]); the count is read here, not in the step
            n_chunks = int(buf["n_chunks"].item())
            return (buf["cand"][:n_chunks].cpu().numpy(), buf["pair"][:n_pos].cpu().numpy(), buf["perm"][:n_pos].cpu().numpy(),
                    buf["chunks"][:n_chunks].cpu().numpy())
        return buf["cand"][:n_chunks].cpu().numpy(), buf["pair"][:n_pos].cpu().numpy()

    def _forget_evaluation(self, arrays=False):
        """A new training or evaluation import: what an earlier import by arrays left behind no longer describes the engine.
        The validation lists kept between calls go only when they are, or were, an array import's (arrays=True: a new one)."""
        if arrays or getattr(self, "_eval_from_arrays", False):
            self._valid_pos = self._valid_rank_dev = self._tc_valid_drawn = self._tc_valid_dev = None
        self._type_lists_from = None      # "arrays" / "derived": the engine's lists did not come from type_constrain.txt
        self._eval_from_arrays = False

    _HOW_TO_SUPPLY_LISTS = ("; supply them with init_evaluation_from_arrays(valid, test, type_lists=...) or derive them from "
                            "the triples with init_evaluation_from_arrays(..., derive_types=True) / derive_type_constraints()")

    def _apply_typed_sampling(self):
        on = bool(self.type_constrained_sampling)
        if on and getattr(self, "_type_lists_from", None) and self.lib.kge_have_type_lists():
            pass      # lists that came by array or by derivation: nothing to read
        elif on:
            if self.in_path is None:
                raise KgeError("type-constrained sampling needs a dataset directory with type_constrain.txt; "
                               "init_from_arrays has no file to read the type lists from" + self._HOW_TO_SUPPLY_LISTS)
            path = self.in_path if self.in_path.endswith("/") else self.in_path + "/"
            if not os.path.exists(path + "type_constrain.txt"):
                raise KgeError("type-constrained sampling: `%stype_constrain.txt` does not exist" % path)
            self.lib.kge_clear_error()
            self.lib.importTypeFiles()
            _lib.raise_if_error(self.lib)
            self._type_lists_from = None
        _lib.check(self.lib.kge_set_typed_sampling(1 if on else 0), self.lib)

    def init_from_arrays(self, ent_total, rel_total, h, t, r, new_batch_total=0):
        """Same as init() with the training triples (file order) given as arrays instead of files."""
        if self.type_constrained_sampling:
            raise KgeError("type-constrained sampling needs a dataset directory with type_constrain.txt; "
                           "init_from_arrays has no file to read the type lists from" + self._HOW_TO_SUPPLY_LISTS +
                           ", then set_type_constrained_sampling(True)")
        self._forget_evaluation(arrays=True)
        h = np.ascontiguousarray(h, dtype=np.int64)
        t = np.ascontiguousarray(t, dtype=np.int64)
        r = np.ascontiguousarray(r, dtype=np.int64)
        self.lib.kge_clear_error()
        self.lib.setBern(self.bern)
        self.lib.setWorkThreads(self.workThreads)
        self.lib.randReset()
        _lib.check(self.lib.kge_import_train_arrays(ent_total, rel_total, len(h), h.ctypes.data, t.ctypes.data,
                                                    r.ctypes.data, new_batch_total), self.lib)
        self.relTotal = self.lib.getRelationTotal()
        self.entTotal = self.lib.getEntityTotal()
        self.trainTotal = self.lib.getTrainTotal_()
        self.testTotal = self.validTotal = 0
        _lib.check(self.lib.kge_set_typed_sampling(0), self.lib)     # (one engine per process: an earlier Config's setting must not linger)
        self.bt = self.lib.getBatchTotal()
        self.set_mini_batch()
        self._alloc_batch_buffers()

    def init_evaluation_from_arrays(self, valid, test, type_lists=None, derive_types=False):
        """What init_link_prediction / init_triple_classification do, with the validation and test triples given as (h, t, r)
        array triples instead of valid2id.txt / test2id.txt (either may be empty); the training triples are the ones the engine
        holds, so it works after init() and after init_from_arrays().  type_lists = (head_off, head_ids, tail_off, tail_ids), the
        per-relation type lists as CSR (relTotal + 1 offsets each), or derive_types=True for the lists the reference writes into
        type_constrain.txt on every launch: each relation's distinct heads and distinct tails over train + valid + test.
        Without either, evaluation runs without typed columns, as without the file.  Ontology lists cannot be given as arrays:
        the classes of a rank stay zero.  From eval_index_device_min triples on the lists are built on the device."""
        if type_lists is not None and derive_types:
            raise KgeError("init_evaluation_from_arrays: give type_lists or derive_types=True, not both")
        cols = [[np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int64) for a in split] for split in (valid, test)]
        for name, split in zip(("valid", "test"), cols):
            if len(split) != 3 or not (len(split[0]) == len(split[1]) == len(split[2])):
                raise KgeError("init_evaluation_from_arrays: %s must be three arrays (h, t, r) of one length" % name)
        (vh, vt, vr), (th, tt, tr) = cols
        self.lib.kge_clear_error()
        _lib.check(self.lib.kge_import_eval_arrays(len(vh), vh.ctypes.data, vt.ctypes.data, vr.ctypes.data,
                                                   len(th), th.ctypes.data, tt.ctypes.data, tr.ctypes.data), self.lib)
        self._forget_evaluation(arrays=True)
        self._eval_from_arrays = True
        self.testTotal = self.lib.getTestTotal()
        self.validTotal = self.lib.getValidTotal()
        self._valid_pos = np.stack([vh, vt, vr]).astype(np.int32)      # validation_link_prediction's positives, in the order given
        if type_lists is not None:
            self.set_type_constraints(*type_lists)
        elif derive_types:
            self.derive_type_constraints()
        self._alloc_tc_buffers()
        if self.type_constrained_sampling:        # the import dropped the lists of an earlier one
            self._apply_typed_sampling()

    def set_type_constraints(self, head_off, head_ids, tail_off, tail_ids):
        """The per-relation type lists as CSR arrays (relTotal + 1 offsets from 0 and the ids, heads then tails), in place of
        type_constrain.txt; each list is sorted on the way in, duplicates kept."""
        arrs = [np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int64) for a in (head_off, head_ids, tail_off, tail_ids)]
        if len(arrs[0]) != self.relTotal + 1 or len(arrs[2]) != self.relTotal + 1:
            raise KgeError("type lists: head_off and tail_off must hold relTotal + 1 = %d offsets" % (self.relTotal + 1))
        if (len(arrs[0]) and len(arrs[1]) != arrs[0][-1]) or (len(arrs[2]) and len(arrs[3]) != arrs[2][-1]):
            raise KgeError("type lists: the last offset must be the number of ids")
        self.lib.kge_clear_error()
        _lib.check(self.lib.kge_set_type_lists(*[a.ctypes.data for a in arrs]), self.lib)
        self._type_lists_from = "arrays"

    def derive_type_constraints(self, write=False):
        """The type lists the reference generates on every launch (main_spark.py n_n()): for every relation the distinct heads
        and the distinct tails over train + valid + test, after any evaluation import (files or arrays).  write=True also
        writes them to <in_path>/type_constrain.txt, with a head and a tail line for EVERY relation."""
        if write and self.in_path is None:
            raise KgeError("derive_type_constraints(write=True) needs an in_path to write type_constrain.txt into")
        _lib.check(self.lib.kge_derive_type_lists(), self.lib)
        self._type_lists_from = "derived"
        if write:
            path = self.in_path if self.in_path.endswith("/") else self.in_path + "/"
            _lib.check(self.lib.kge_write_type_constraints((path + "type_constrain.txt").encode()), self.lib)

    def type_constraints(self):
        """The engine's current type lists as CSR: (head_off, head_ids, tail_off, tail_ids), int64."""
        R = self.lib.getRelationTotal()
        head_off, tail_off = np.zeros(R + 1, np.int64), np.zeros(R + 1, np.int64)
        self.lib.kge_clear_error()
        _lib.check(self.lib.kge_get_type_lists(head_off.ctypes.data, None, tail_off.ctypes.data, None), self.lib)
        head_ids, tail_ids = np.zeros(int(head_off[-1]), np.int64), np.zeros(int(tail_off[-1]), np.int64)
        _lib.check(self.lib.kge_get_type_lists(head_off.ctypes.data, head_ids.ctypes.data, tail_off.ctypes.data, tail_ids.ctypes.data), self.lib)
        return head_off, head_ids, tail_off, tail_ids

    def _alloc_batch_buffers(self):
        # Config.py:172-180
        self.batch_seq_size = self.batch_size * (1 + self.negative_ent + self.negative_rel)
        self.batch_h = np.zeros(self.batch_seq_size, dtype=np.int64)
        self.batch_t = np.zeros(self.batch_seq_size, dtype=np.int64)
        self.batch_r = np.zeros(self.batch_seq_size, dtype=np.int64)
        self.batch_y = np.zeros(self.batch_seq_size, dtype=np.float32)
        self.batch_h_addr = self.batch_h.__array_interface__['data'][0]
        self.batch_t_addr = self.batch_t.__array_interface__['data'][0]
        self.batch_r_addr = self.batch_r.__array_interface__['data'][0]
        self.batch_y_addr = self.batch_y.__array_interface__['data'][0]

    def set_mini_batch(self):
        '''
        Set mini batch used during training (Config.py:189-210)
        '''
        tot = self.bt if self.bt > 0 else self.trainTotal
        if self.nbatches > 0:
            self.batch_size = int(tot / self.nbatches)
        else:
            self.batch_size = tot
            while self.batch_size > 9999:
                self.batch_size = int(self.batch_size / 10)
            self.nbatches = int(tot / self.batch_size)
        print("Batch size is {}".format(self.batch_size))
        print("Number of batches: {}".format(self.nbatches))

    # ------------------------------------------------------------------------------------------
    # getters / setters (Config.py:213-340, 425-429)
    # ------------------------------------------------------------------------------------------
    def get_ent_total(self):
        return self.entTotal

    def get_rel_total(self):
        return self.relTotal

    def set_opt_method(self, method):
        self.opt_method = method

    def set_test_link_prediction(self, flag):
        self.test_link_prediction = flag

    def set_test_relation_prediction(self, flag):
        """test() also reports the rel* relation-prediction metrics (relation_prediction); init() then imports the test files."""
        self.test_relation_prediction = flag

    def set_test_triple_classification(self, flag):
        self.test_triple_classification = flag

    def set_valid_triple_classification(self, flag):
        self.valid_triple_classification = flag

    def set_alpha(self, alpha):
        self.alpha = alpha

    def set_in_path(self, path):
        self.in_path = path

    def set_out_files(self, path):
        self.out_path = path

    def set_bern(self, bern):
        self.bern = bern

    def set_dimension(self, dim):
        self.hidden_size = dim
        self.ent_size = dim
        self.rel_size = dim

    def set_ent_dimension(self, dim):
        self.ent_size = dim

    def set_rel_dimension(self, dim):
        self.rel_size = dim

    def set_train_times(self, times):
        self.train_times = times

    def set_nbatches(self, nbatches):
        self.nbatches = nbatches

    def set_margin(self, margin):
        self.margin = margin

    def set_ent_neg_rate(self, rate):
        self.negative_ent = rate

    def set_rel_neg_rate(self, rate):
        self.negative_rel = rate

    def set_import_files(self, path):
        self.importName = path

    def set_export_files(self, path):
        self.exportName = path

    def set_work_threads(self, threads):
        """Number of VIRTUAL sampler threads (rng streams / batch slices, Setting.h:36-39).  The
        reference hard-codes 8 (Config.py:65); data-parallel ranks split them."""
        self.workThreads = threads

    def set_model(self, model):
        self.model = model

    # ------------------------------------------------------------------------------------------
    # sampling: Base.so-compatible host path (Config.py:343-347)
    # ------------------------------------------------------------------------------------------
    def sampling(self):
        '''
        Call the engine for batch sampling into the numpy buffers (same bits as the reference)
        '''
        self.lib.kge_clear_error()
        self.lib.sampling(self.batch_h_addr, self.batch_t_addr, self.batch_r_addr, self.batch_y_addr,
                          self.batch_size, self.negative_ent, self.negative_rel)
        _lib.raise_if_error(self.lib)

    # ------------------------------------------------------------------------------------------
    # "session": parameters, optimiser state, train / test steps
    # ------------------------------------------------------------------------------------------
    def set_model_and_session(self, model):
        '''
        Create the model's device tables and the optimiser state (Config.py:447-461 +
        distribute_training.create_model, :74-105).
        '''
        import torch
        self.model = model
        # which path the steps will take (step_plan.py), decided before anything is created: a row-sharded entity table is drawn
        # shard-sized.  `sparse_rows` None = automatic, True / False = the caller's wish; `use_counts` likewise a wish until here
        n_neg = self.negative_ent + self.negative_rel
        probe = model(config=self, define=False)
        p = self._plan = step_plan.plan(
            probe.model_id, self.opt_method, getattr(self, "sparse_rows", None), getattr(self, "use_counts", True),
            self.lib.kge_transe_counts_supported(ctypes.byref(probe.descriptor()), n_neg), self.entTotal, self.relTotal,
            self.hidden_size, self.batch_size, n_neg, getattr(self, "sparse_threshold_bytes", None), self.adagrad_initial_accumulator,
            shared_chunk=self._shared_chunk, negative_rel=self.negative_rel, by_relation=self._shared_by_relation,
            typed=bool(self._shared_chunk and self.type_constrained_sampling),
            shared_float_supported=self.lib.kge_shared_float_supported(ctypes.byref(probe.descriptor()), self.negative_ent),
            shared_transd_supported=self.lib.kge_shared_transd_supported(ctypes.byref(probe.descriptor()), self.negative_ent),
            shared_transr_supported=self.lib.kge_shared_transr_supported(ctypes.byref(probe.descriptor()), self.negative_ent),
            in_chunk=self._shared_in_chunk, table_dtype=getattr(self, "_table_dtype", "fp32"),
            bf16_supported=self.lib.kge_bf16_tables_supported(ctypes.byref(probe.descriptor()), n_neg) if self._bf16 else 0,
            bf16_shared_supported=self.lib.kge_bf16_shared_supported(ctypes.byref(probe.descriptor()), self.negative_ent + self._shared_in_chunk)
            if self._bf16 and self._shared_chunk else 0)
        if self._bf16 and self._shared_chunk:      # (a shape the plan takes: the two hashes must be keyed apart)
            step_plan.check_bf16_shared_seeds(self._table_seed, self._shared_seed)
        self._drop_eval_view()
        self.use_counts, self.sparse_rows, self.sparse_inplace = p.use_counts, p.sparse_rows, p.sparse_inplace
        self._adam, self._lazy_adam, self._adagrad = p.adam, p.lazy_adam, p.adagrad
        self._row_adagrad = p.row_adagrad
        self._has_slots, self._rows_rule = p.has_slots, p.rows_rule
        self._refuse_shared_ranks()
        self._refuse_bf16_ranks()
        self._shard_plan = self._plan_entity_shard(probe.model_id)
        self.trainModel = self.model(config=self, define=True)
        m = self.trainModel
        self._desc = m.descriptor()
        self._tables = [m.parameter_lists[n] for n in m.table_names]
        self._grads = [] if (self.sparse_rows or self.sparse_inplace) else [torch.zeros_like(t) for t in self._tables]
        if self._has_slots:
            self._adam_m = [torch.zeros_like(t) for t in self._tables]
            self._adam_v = [torch.zeros_like(t) for t in self._tables]
            self._beta1_power = np.float32(self.adam_beta1)
            self._beta2_power = np.float32(self.adam_beta2)
        if self._adagrad:      # shaped like the tables: a row-sharded entity table (Model.embedding_def) gets a shard-sized accumulator
            self._adagrad_acc = [torch.full_like(t, float(self.adagrad_initial_accumulator)) for t in self._tables]
        if self._row_adagrad:  # ONE float per table row (TransR's transfer_matrix: per relation); shard-sized where the entity table is
            self._rowadagrad_acc = [torch.full((t.shape[0],), float(self.adagrad_initial_accumulator), dtype=torch.float32, device=t.device)
                                    for t in self._tables]
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._refresh_pointers()
        self._dist_ready = 0
        self._dev_batch = None
        self._dev_positives = None     # the shared-negatives step's batch: positives alone (_sample_positives)
        self._dev_pack = None          # the sampler's packed negatives of the two batch slots (_pack_for)
        self._batch_pack = 0           # pack of the batch the current step trains on (device pointer; 0 = none)
        self._prefetched_pack = 0      # ... of the batch drawn ahead
        self._dev_batch2 = None
        self._side_stream = None
        self._prefetched = None
        self.global_step = 0
        self._sparse_buf = None
        # TransE steps with fewer gradient rows than this take the single fused fp32-atomic kernel (launch-bound
        # regime, tools/sweep_paths.py); 0 = always the exact, run-to-run reproducible count pipeline
        self.counts_min_records = int(getattr(self, "counts_min_records",
                                              os.environ.get("KGE_COUNTS_MIN_RECORDS", 1 << 16)))
        # None = automatic: on in data-parallel runs (batch i+1 is drawn while step i's gradient exchange waits on the wire) and,
        # at 1 GPU, on the sign-count path, where the sampler starts right behind the emit kernel and runs beside the small
        # kernels after it (measured +4 %); off on the other 1-GPU paths (there it only competes with the step's own kernels)
        self.prefetch_sampling = getattr(self, "prefetch_sampling", None)
        self._prefetch_auto = self.prefetch_sampling is None      # (init_distributed decides again once the world size is known)
        if self._prefetch_auto:
            self.prefetch_sampling = self._prefetch_default()
        if self.use_counts and not self.sparse_rows:
            self._counts = torch.zeros((self.entTotal + self.relTotal, self.hidden_size), dtype=torch.int32,
                                       device=self.device)
        self._setup_partition()

    def _plan_entity_shard(self, model_id):
        """If this process already belongs to a torch.distributed world of N > 1 ranks and the step will be the table-sharded
        sparse one (step_plan.shards_at_creation), the rows [lo, hi) of the entity table this rank will own:
        the model then draws ONLY those rows (Model.embedding_def) instead of the whole table that train_paths.setup_shards
        would cut down -- 102 GB per rank at BASELINE config #5.  None otherwise (the table is created whole, as before)."""
        try:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                return None
            W, g = dist.get_world_size(), dist.get_rank()
        except Exception:
            return None
        if not step_plan.shards_at_creation(self._plan, model_id, W, self.hidden_size):
            return None
        from .parallel import chunk_size
        chunk = chunk_size(self.entTotal, W)
        return dict(world=W, rank=g, chunk=chunk, lo=min(g * chunk, self.entTotal), hi=min((g + 1) * chunk, self.entTotal))

    # --- data-parallel partition: rank g owns virtual threads [g*W/G, (g+1)*W/G) ---
    def init_distributed(self, process_group=None):
        """Join the (already initialised) torch.distributed world: one process per GPU, RCCL."""
        import torch.distributed as dist
        self._pg = process_group
        self.rank = dist.get_rank(process_group)
        self.world_size = dist.get_world_size(process_group)
        self._refuse_bf16_ranks()
        if self.trainModel is not None:
            self._setup_partition()
        if getattr(self, "_prefetch_auto", getattr(self, "prefetch_sampling", None) is None):
            self.prefetch_sampling = self._prefetch_default()

    def _prefetch_default(self):
        if self.trainModel is None:      # init_distributed before a model is set: nothing is known but the caller's `sparse_rows` wish
            return bool(self.world_size > 1 or not getattr(self, "sparse_rows", False))
        p = self._plan
        n_neg = self.negative_ent + self.negative_rel
        counts_path = step_plan.large_counts_step(p, self.batch_size, n_neg, self.counts_min_records, self.world_size)
        pair_path = bool(self.lib.kge_pair_path_active(ctypes.byref(self._desc), max(self._n_local, 1) if hasattr(self, "_n_local") else self.batch_size, n_neg))
        transr = self.trainModel.model_id == _lib.TRANSR
        dense_one_gpu = not p.sparse_rows and not p.sparse_inplace
        return bool(self.world_size > 1 or counts_path or pair_path or transr or dense_one_gpu)

    @property
    def _dp(self):
        """Does a step go through the data-parallel exchange?  More than one rank -- or `force_data_parallel` on a one-rank
        process group: the rehearsal of the RCCL path (collectives on device memory, asynchronous work handles, the in-place
        all-gather) on a box with a single GPU; results equal the plain single-process step bit for bit."""
        return self.world_size > 1 or bool(getattr(self, "force_data_parallel", False))

    def _setup_partition(self):
        from .parallel import thread_range
        lo, hi = thread_range(self.rank, self.world_size, self.workThreads)
        self._thread_lo, self._thread_hi = lo, hi
        self._refuse_shared_ranks()
        self._refuse_bf16_ranks()
        first = ctypes.c_int64(0)
        self._n_local = self.lib.kge_slice_positions(self.batch_size, lo, hi, ctypes.byref(first))
        self._first_pos = first.value
        if self._dp and self.trainModel is not None and getattr(self, "_dist_ready", 0) != self.world_size:
            if self._adagrad and not (self.sparse_rows or self.sparse_inplace):
                raise KgeError("TransR with Adagrad is single-process only: the data-parallel dense step has no flat accumulator "
                               "for its reduce-scatter exchange")
            if self._row_adagrad and not (self.sparse_rows or self.sparse_inplace):
                raise KgeError("TransR with RowAdagrad is single-process only: the data-parallel dense step cuts its flat buffer "
                               "anywhere, and the rule needs a row's complete gradient")
            if self.sparse_inplace:
                pass          # replicated tables, the step's gradient records all-gathered (train_paths.records_step): nothing to lay out
            elif self.sparse_rows:
                train_paths.setup_shards(self)
            else:
                train_paths.setup_flat_buffers(self)
            self._dist_ready = self.world_size

    def _refresh_pointers(self):
        self.lib.kge_set_option(b"tables_changed", 1)
        self._tab_ptrs = _lib.table_ptrs([t.data_ptr() for t in self._tables])
        self._grad_ptrs = _lib.table_ptrs([g.data_ptr() for g in self._grads])
        self._numel = (ctypes.c_int64 * _lib.KGE_MAX_TABLES)(*[t.numel() for t in self._tables])
        if self._has_slots:
            self._adam_m_ptrs = _lib.table_ptrs([t.data_ptr() for t in self._adam_m])
            self._adam_v_ptrs = _lib.table_ptrs([t.data_ptr() for t in self._adam_v])
        if self._adagrad:
            self._adagrad_ptrs = _lib.table_ptrs([t.data_ptr() for t in self._adagrad_acc])
        if self._row_adagrad:
            self._rowadagrad_ptrs = _lib.table_ptrs([t.data_ptr() for t in self._rowadagrad_acc])
            self._table_rows = (ctypes.c_int64 * _lib.KGE_MAX_TABLES)(*[t.shape[0] for t in self._tables])
            self._row_len = (ctypes.c_int64 * _lib.KGE_MAX_TABLES)(*[t.numel() // max(t.shape[0], 1) for t in self._tables])
        self._rule = train_paths.RowsRule(self)      # (it holds these pointers)

    def _stream(self):
        """The current HIP stream of this Config's device, as the C ABI takes it.  Read through the raw accessor: building a
        torch.cuda.Stream object per call (torch.cuda.current_stream()) was 60 % of the host time of a step at the reference's
        batch sizes, where the host, not the GPU, set the step time (tools/host_bound_small.py)."""
        import torch
        if getattr(self, "_dev_index_of", None) != self.device:       # (callers may set con.device after construction)
            d = torch.device(self.device)
            self._dev_index = d.index if d.index is not None else torch.cuda.current_device()
            self._dev_index_of = self.device
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)      # (a private accessor: fall back to the public object if it ever goes)
        return ctypes.c_void_p(raw(self._dev_index) if raw is not None else torch.cuda.current_stream().cuda_stream)

    def _ensure_dev_batch(self, stride):
        import torch
        n = stride * (1 + self.negative_ent + self.negative_rel)
        if self._dev_batch is None or self._dev_batch.shape[2] != n:
            self._dev_batch = torch.zeros((2, 3, n), dtype=torch.int32, device=self.device)  # two slots: double buffer
        return self._dev_batch

    def _pack_for(self, slot):
        """Device pointer of batch slot `slot`'s packed negatives (include/kge_mi355.h kge_sampling_device_packed), 0 = this
        configuration's step reads none: only the TransE sign-count step does, and the engine says for which batch shapes
        (kge_emit_pack_words; option emit_pack).  Allocated next to the batch: two slots of n_local << kshift words."""
        import torch
        n_neg = self.negative_ent + self.negative_rel
        if not step_plan.large_counts_step(self._plan, self.batch_size, n_neg, self.counts_min_records, self.world_size):
            return 0
        words = int(self.lib.kge_emit_pack_words(self._n_local, self.negative_ent, self.negative_rel, self.hidden_size))
        if words <= 0:
            return 0
        if self._dev_pack is None or self._dev_pack.shape[1] != words:
            self._dev_pack = torch.zeros((2, words), dtype=torch.int32, device=self.device)
        return self._dev_pack[slot].data_ptr()

    def sample_device(self, slot=0):
        """Sample this rank's slice of the next batch on the device; returns (int32[3,n] tensor, n_pos)."""
        stride = max(self._n_local, 1)
        buf = self._ensure_dev_batch(stride)[slot]
        nl = ctypes.c_int64(0)
        pack = self._pack_for(slot)
        _lib.check(self.lib.kge_sampling_device_packed(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), pack or None,
                                                       self.batch_size, self.negative_ent, self.negative_rel,
                                                       self._thread_lo, self._thread_hi, stride, ctypes.byref(nl),
                                                       self._stream()), self.lib)
        self._batch_pack = pack        # (a pack goes with the batch drawn in the same call, and with no other)
        return buf, nl.value

    def _sample_positives(self):
        """This rank's positives of the next batch alone (the sampler at negRate = 0, one draw per positive): (int32 [3, stride]
        tensor, n_pos) -- the shared-negatives step's batch."""
        import torch
        stride = max(self._n_local, 1)
        if getattr(self, "_dev_positives", None) is None or self._dev_positives.shape[1] != stride:
            self._dev_positives = torch.zeros((3, stride), dtype=torch.int32, device=self.device)
        buf = self._dev_positives
        nl = ctypes.c_int64(0)
        _lib.check(self.lib.kge_sampling_device(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), self.batch_size, 0, 0,
                                                self._thread_lo, self._thread_hi, stride, ctypes.byref(nl), self._stream()), self.lib)
        return buf, nl.value

    def _next_sampled_batch(self):
        """The batch for this step, sampled one step ahead on a side stream: the sampler depends on the rng
        streams and the dataset only, never on the parameters, so batch i+1 is drawn while step i's
        reduction / gradient exchange / update run.  Same batches, same order, same bits."""
        import torch
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream()
            self._slot = 0
            self._prefetched = None
            self.lib.kge_set_option(b"record_emit_event", 1)
        if self._prefetched is None:
            dev, n_pos = self.sample_device(self._slot)
        else:
            dev, n_pos, ev = self._prefetched
            self._batch_pack = self._prefetched_pack
            if ev is not None:            # (None: drawn on this stream by a sampler that rode in a launch of the step)
                torch.cuda.current_stream().wait_event(ev)
        return dev, n_pos

    def _attach_next_batch(self):
        """Arm the sampler of the NEXT batch so that it rides in this step's bucket-scatter launch (kge_sampling_attach): the
        sign-count path's way of drawing batch i+1 during step i -- one stream, no events.  Call _flush_next_batch() once the
        step's forward launches are enqueued."""
        stride = max(self._n_local, 1)
        self._slot ^= 1
        buf = self._ensure_dev_batch(stride)[self._slot]
        nl = ctypes.c_int64(0)
        pack = self._pack_for(self._slot)
        _lib.check(self.lib.kge_sampling_attach_packed(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), pack or None,
                                                       self.batch_size, self.negative_ent, self.negative_rel, self._thread_lo,
                                                       self._thread_hi, stride, ctypes.byref(nl), self._stream()), self.lib)
        self._prefetched = (buf, nl.value, None)
        self._prefetched_pack = pack

    def _flush_next_batch(self):
        _lib.check(self.lib.kge_sampling_flush(self._stream()), self.lib)

    def _prefetch_next_batch(self, behind_emit=False):
        """behind_emit=True (the sign-count path): the side stream waits for THIS step's emit kernel only -- the one
        bandwidth-bound kernel of the step, which a concurrent sampler would slow down by what it takes -- and the sampler
        then runs beside the small latency-bound kernels after it (bucketing, segmented sum, apply).  The other slot's last
        readers (the previous step's kernels) are older than that emit kernel."""
        import torch
        main = torch.cuda.current_stream()
        done = None
        if not behind_emit:
            done = torch.cuda.Event()
            done.record(main)                  # the consumers of the OTHER slot (previous step) were enqueued before this
        self._slot ^= 1
        with torch.cuda.stream(self._side_stream):
            if behind_emit:
                rc = _lib.check(self.lib.kge_stream_wait_emit(ctypes.c_void_p(self._side_stream.cuda_stream)), self.lib)
                if rc == _lib.NO_EVENT:            # this step recorded no emit event: wait for everything enqueued so far
                    done = torch.cuda.Event()
                    done.record(main)
            if done is not None:
                self._side_stream.wait_event(done)  # slot reuse: its last reader is older than `done`
            dev, n_pos = self.sample_device(self._slot)
            ev = torch.cuda.Event()
            ev.record(self._side_stream)
        self._prefetched = (dev, n_pos, ev)
        self._prefetched_pack = self._batch_pack

    def forward_backward(self, dev_batch, n_pos, stride, denom, sampler_shaped=False):
        """Add dLoss/dTables of the batch into the gradient accumulators; loss -> self._loss.
        sampler_shaped=True (a device-sampled batch): paths with a separate exact pass for other batches skip it
        (include/kge_mi355.h kge_forward_backward_sampled)."""
        fn = self.lib.kge_forward_backward_sampled if sampler_shaped else self.lib.kge_forward_backward
        _lib.check(fn(ctypes.byref(self._desc), self._tab_ptrs,
                                                 dev_batch[0].data_ptr(), dev_batch[1].data_ptr(),
                                                 dev_batch[2].data_ptr(), n_pos,
                                                 self.negative_ent + self.negative_rel, stride, denom,
                                                 self._grad_ptrs, self._loss.data_ptr(), self._stream()), self.lib)

    def _adam_lr_t(self):
        f = np.float32
        return f(f(self.alpha) * np.sqrt(f(1) - self._beta2_power, dtype=np.float32) / (f(1) - self._beta1_power))

    def _adam_advance(self):
        f = np.float32
        self._beta1_power = f(self._beta1_power * f(self.adam_beta1))
        self._beta2_power = f(self._beta2_power * f(self.adam_beta2))

    def apply_gradients(self, own=False, piece=0):
        """GradientDescentOptimizer / AdamOptimizer on the summed gradients (distribute_training.py:95-101).
        own=True (data-parallel): on this rank's chunk of the flat parameter buffer only, from its reduce-scattered
        gradient chunk."""
        st = self._stream()
        if own:       # one piece of this rank's share (train_step's exchange loop calls it per piece and advances Adam once)
            if self._adagrad:
                raise KgeError("TransR with Adagrad is single-process only")
            if self._row_adagrad:
                raise KgeError("TransR with RowAdagrad is single-process only")
            lo, hi = self._piece_own[piece]
            n = hi - lo
            if hi > self._loss_tail:
                n -= 4                                        # the spare tail slot (it holds the loss, not a parameter)
            p, g = self._flat_p.data_ptr() + 4 * lo, self._grads_own.data_ptr() + 4 * piece * self._own_len
            if self._adam:
                _lib.check(self.lib.kge_adam_update(p, self._flat_m.data_ptr() + 4 * lo, self._flat_v.data_ptr() + 4 * lo, g, n,
                                                    float(self._adam_lr_t()), self.adam_beta1, self.adam_beta2,
                                                    self.adam_epsilon, st), self.lib)
                self._opt_state_synced = False
            else:
                _lib.check(self.lib.kge_sgd_update(p, g, n, float(self.alpha), st), self.lib)
            return
        elif self._adam:
            _lib.check(self.lib.kge_adam_update_tables(len(self._tables), self._tab_ptrs, self._adam_m_ptrs, self._adam_v_ptrs,
                                                       self._grad_ptrs, self._numel, float(self._adam_lr_t()), self.adam_beta1,
                                                       self.adam_beta2, self.adam_epsilon, st), self.lib)
            self._adam_advance()
        elif self._adagrad:     # (TransR: every other model takes a touched-rows path under Adagrad)
            _lib.check(self.lib.kge_adagrad_update_tables(len(self._tables), self._tab_ptrs, self._adagrad_ptrs, self._grad_ptrs,
                                                          self._numel, float(self.alpha), st), self.lib)
        elif self._row_adagrad:  # (TransR likewise; a row of transfer_matrix is one relation's whole matrix)
            _lib.check(self.lib.kge_rowadagrad_update_tables(len(self._tables), self._tab_ptrs, self._rowadagrad_ptrs, self._grad_ptrs,
                                                             self._table_rows, self._row_len, float(self.alpha), st), self.lib)
        else:
            _lib.check(self.lib.kge_sgd_update_tables(len(self._tables), self._tab_ptrs, self._grad_ptrs, self._numel,
                                                      float(self.alpha), st), self.lib)
        self.global_step += 1

    def comm_fence(self, kind):
        """Two RCCL communicators live in a data-parallel process: torch's process group ("pg": the sharded step, optimizer-state
        gathers, evaluation reductions, the caller's own barriers) and the engine's own (parallel.StreamRccl, "nat": the dense
        step's reduce-scatter / all-gather on the engine's stream).  Collectives of two communicators must never be in flight
        together on a device: each spins on its peers, and two ranks that get them scheduled in opposite order wait on each other
        for ever.  The rule enforced here: every collective is issued through ONE communicator per step path, and whenever the
        communicator CHANGES (first step after a checkpoint gather, an evaluation, ...) the device is drained first -- every
        collective this rank has enqueued so far has then completed, so its peers have all entered it, before a collective of
        the other communicator is enqueued.  Every rank runs the same program, so all ranks fence at the same points.  Call it with
        "pg" before using torch.distributed collectives of your own between training steps."""
        last = getattr(self, "_last_comm", None)
        if last is not None and last != kind:
            import torch
            torch.cuda.synchronize(self.device)
        self._last_comm = kind

    def _stream_rccl(self):
        return train_paths.stream_rccl(self)

    def last_exchange_sizes(self):
        """What this rank's most recent step on a row-sharded entity table (train_paths.sharded_step / shared_sharded_step)
        exchanged, as a dict of row counts: rows_requested (entity rows it fetched from their owners), rows_served (rows it
        gathered for others), records_sent (entity gradient records it sent to the rows' owners), records_received.  Read-only;
        None before the first such step."""
        sizes = getattr(self, "_exchange_sizes", None)
        return dict(sizes) if sizes is not None else None

    def sync_optimizer_state(self):
        """Data-parallel Adam keeps m and v current on their owner only; gather them before they are read as whole tables
        (checkpoints)."""
        if self._dp and self._adam and not self.sparse_rows and not getattr(self, "_opt_state_synced", True):
            from .parallel import all_gather_chunks
            self.comm_fence("pg")
            for (slo, shi), (lo, hi) in zip(self._piece_seg, self._piece_own):
                all_gather_chunks(self._flat_m[slo:shi], self._flat_m[lo:hi], self._pg)
                all_gather_chunks(self._flat_v[slo:shi], self._flat_v[lo:hi], self._pg)
            self._opt_state_synced = True

    def train_step(self, batch_h=None, batch_t=None, batch_r=None, batch_y=None, sync=True):
        '''
        Perform a single training step (Config.py:464-475 / distribute_training.py:274-282).
        With no arguments the batch is sampled on the device; with the reference's four arrays the
        given batch (layout of Config.batch_h/t/r) is trained on.  Returns the loss (float) when
        sync=True, else the device scalar.
        '''
        import torch
        n_neg = self.negative_ent + self.negative_rel
        if self._bf16:
            self._refuse_bf16_ranks()
            self._drop_eval_view()      # the view is of the tables before this step
        if getattr(self, "_ent_is_shard", False) and not hasattr(self, "_shard"):
            raise KgeError("the entity table was created as this rank's shard of a row-sharded table (the process belongs to a "
                           "torch.distributed world): call init_distributed() before training")
        if self._shared_chunk:
            if batch_h is not None:
                raise KgeError("shared negatives: a hand-fed batch is refused (the step draws its own positives and hashes its "
                               "candidates from the global step)")
            self._refuse_shared_ranks(stepping=True)
            dev, n_pos = self._sample_positives()
            step = (train_paths.shared_sharded_step if self._dp else
                    train_paths.shared_grouped_step if self._shared_by_relation else train_paths.shared_step)
            step(self, dev, n_pos, max(self._n_local, 1), self.batch_size * (self.negative_ent + self._shared_in_chunk))
            self.trainModel.loss = self._loss
            return float(self._loss.item()) if sync else self._loss
        if batch_h is None:
            dev, n_pos = self._next_sampled_batch() if self.prefetch_sampling else self.sample_device()
            stride = max(self._n_local, 1)
            pack = self._batch_pack        # written by the sampler call that drew `dev`
        else:
            pack = 0
            if self._dp:      # (also a one-rank group under force_data_parallel: the sharded step has no check for hand-made negatives)
                raise KgeError("feeding a host batch is single-process only")
            host = np.stack([np.asarray(batch_h), np.asarray(batch_t), np.asarray(batch_r)]).astype(np.int32)
            self._check_ids(host)
            dev = torch.from_numpy(host).to(self.device)
            n_pos = host.shape[1] // (1 + n_neg)
            stride = n_pos
        sampled = batch_h is None
        denom = self.batch_size * n_neg if sampled else n_pos * n_neg
        ahead = sampled and self.prefetch_sampling      # draw the next batch during this step
        if self.sparse_inplace or self.sparse_rows:
            if self.sparse_inplace and self._dp:
                train_paths.records_step(self, dev, n_pos, stride, denom)
            elif self.sparse_inplace:
                train_paths.inplace_step(self, dev, n_pos, stride, denom, hand_fed=not sampled)
            elif self._dp:
                train_paths.sharded_step(self, dev, n_pos, stride, denom)
            else:
                train_paths.sparse_step(self, dev, n_pos, stride, denom, check_shape=not sampled)
            if ahead:
                self._prefetch_next_batch()
        elif step_plan.large_counts_step(self._plan, self.batch_size if sampled else n_pos, n_neg, self.counts_min_records, self.world_size):
            # (small steps are launch-bound: there the single fused atomic kernel of the dense step beats the multi-stage count pipeline)
            train_paths.counts_step(self, dev, n_pos, stride, denom, sampled, pack, ahead)
        else:
            train_paths.dense_step(self, dev, n_pos, stride, denom, sampled, ahead)
        self.trainModel.loss = self._loss
        return float(self._loss.item()) if sync else self._loss

    def persistent_supported(self):
        """Can train_steps() run its steps inside one persistent launch (csrc/persist.hip)?  Single process, the dense
        fp32-accumulator path of TransE / TransH / TransD at a launch-latency-bound step size.  Not with type-constrained
        sampling: the persistent kernel has the untyped sampler only."""
        if self.type_constrained_sampling or self._adagrad or self._row_adagrad or self._shared_chunk:       # (persist.hip has the SGD and Adam sweeps only, and independent negatives)
            return False
        if self._dp or self.sparse_rows or self.sparse_inplace or self.hidden_size > 256:
            return False
        if self.trainModel.model_id not in (_lib.TRANSE, _lib.TRANSH, _lib.TRANSD):
            return False
        n_neg = self.negative_ent + self.negative_rel
        if step_plan.large_counts_step(self._plan, self.batch_size, n_neg, self.counts_min_records, 1):
            return False      # TransE at a large step: the exact integer-count pipeline is the faster path
        slots = {_lib.TRANSE: 3 + n_neg, _lib.TRANSH: 4 + n_neg, _lib.TRANSD: 6 + 2 * n_neg}[self.trainModel.model_id]
        return self.batch_size * slots < int(getattr(self, "persistent_max_rows", 1 << 16))

    def persistent_preferred(self):
        """Is the persistent launch the FASTER way to run this configuration?  Measured (profiles/r03_a_other_configs.jsonl and the
        bench line's config-#1 leg): TransE at its auto batch 26-27 us/step against 27-29 as separate launches (round 2: 27.8
        against 35.2 -- the sampler now rides in the forward/backward launch and the host side of a step is cheaper); TransH /
        TransD steps are bound by the fp32-atomic rate of their gradient rows either way and the separate launches are quicker
        (66-70 vs 77-80 us at config #3's batch)."""
        return self.persistent_supported() and self.trainModel.model_id == _lib.TRANSE

    def train_steps(self, n_steps, persistent=None):
        """`n_steps` iterations of the training loop body (distribute_training.py:267-283): sample, forward / backward,
        update.  Returns the losses (numpy float32 [n_steps]).  Where persistent_preferred() (or with persistent=True where
        persistent_supported()), all the steps run inside ONE persistent launch; otherwise as n_steps calls of train_step()."""
        import torch
        n_steps = int(n_steps)
        if n_steps <= 0:
            return np.zeros(0, np.float32)
        use = self.persistent_preferred() if persistent is None else bool(persistent)
        if use and self._bf16:
            raise KgeError("train_steps(persistent=True): bf16 table storage has no persistent-launch path (the persistent kernel "
                           "reads and sweeps fp32 tables)")
        if use and not self.persistent_supported():
            raise KgeError("train_steps(persistent=True): this configuration has no persistent-launch path" +
                           (" (type-constrained sampling is on: the persistent kernel samples untyped negatives only)"
                            if self.type_constrained_sampling else "") +
                           (" (shared negatives are on: the persistent kernel draws every negative for one positive)"
                            if self._shared_chunk else ""))
        if not use:
            out = [self.train_step(sync=False).clone() for _ in range(n_steps)]   # (the loss scalar is one reused device buffer)
            return torch.stack([o.reshape(()) for o in out]).cpu().numpy()
        if self._prefetched is not None:
            raise KgeError("train_steps: a batch was sampled ahead by train_step(); use one or the other in a run")
        f = np.float32
        lr = np.empty(n_steps, np.float32)
        powers = None
        if self._adam:
            saved = (self._beta1_power, self._beta2_power)
            for i in range(n_steps):
                lr[i] = self._adam_lr_t()
                self._adam_advance()
            powers = (self._beta1_power, self._beta2_power)
            self._beta1_power, self._beta2_power = saved       # committed below, once the launch is known to have completed
        else:
            lr[:] = f(self.alpha)
        losses = torch.empty(n_steps, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.kge_train_steps_persistent(
            ctypes.byref(self._desc), self._tab_ptrs, self._grad_ptrs, self._adam_m_ptrs if self._adam else None,
            self._adam_v_ptrs if self._adam else None, self.batch_size, self.negative_ent, self.negative_rel, n_steps,
            1 if self._adam else 0, lr.ctypes.data, self.adam_beta1, self.adam_beta2, self.adam_epsilon, losses.data_ptr(),
            self._stream()), self.lib)
        out = losses.cpu().numpy()          # synchronises: the launch has drained
        flag = ctypes.c_int32(0)
        _lib.check(self.lib.kge_persistent_aborted(ctypes.byref(flag)), self.lib)
        if flag.value:
            raise KgeError("persistent training launch aborted: a grid barrier did not complete (is another process holding "
                           "compute units of this GPU?); the tables are in an intermediate state")
        if powers is not None:
            self._beta1_power, self._beta2_power = powers
        self.global_step += n_steps
        self._loss.copy_(losses[-1:])
        self.trainModel.loss = self._loss
        return out

    def _desc_with(self, **fields):
        """A copy of the model descriptor with some fields replaced (row spaces of a cache / a shard)."""
        d = self._desc
        vals = {name: getattr(d, name) for name, _ in d._fields_}
        vals.update(fields)
        return _lib.ModelDesc(*[vals[name] for name, _ in d._fields_])

    def sparse_row_gradients(self):
        """(rows int32[n], counts int32[n, D]) of the last sparse step: the touched rows (entity rows first, relation
        rows offset by entTotal) and their integer sign counts (complete only with sparse_fused = False)."""
        n = int(self._sparse_buf["n_rows"].item())
        return self._sparse_buf["rows"][:n], self._sparse_buf["row_counts"][:n]

    def forward_counts(self, dev_batch, n_pos, stride, denom, sampler_shaped=False, pack=0):
        """TransE sign-count forward/backward: exact int32 gradient counts -> self._counts.
        sampler_shaped=True (a device-sampled batch): no residual pass is needed (include/kge_mi355.h).
        pack: the packed negatives the sampler wrote for THIS batch (_pack_for), 0 = none."""
        if sampler_shaped and pack:
            _lib.check(self.lib.kge_transe_forward_counts_packed(
                ctypes.byref(self._desc), self._tables[0].data_ptr(), self._tables[1].data_ptr(),
                dev_batch[0].data_ptr(), dev_batch[1].data_ptr(), dev_batch[2].data_ptr(), pack, n_pos,
                self.negative_ent + self.negative_rel, stride, denom, self._counts.data_ptr(),
                self._loss.data_ptr(), self._stream()), self.lib)
            return
        resid = (None, None) if sampler_shaped else (self._grads[0].data_ptr(), self._grads[1].data_ptr())
        _lib.check(self.lib.kge_transe_forward_counts(
            ctypes.byref(self._desc), self._tables[0].data_ptr(), self._tables[1].data_ptr(),
            dev_batch[0].data_ptr(), dev_batch[1].data_ptr(), dev_batch[2].data_ptr(), n_pos,
            self.negative_ent + self.negative_rel, stride, denom, self._counts.data_ptr(),
            resid[0], resid[1], self._loss.data_ptr(), self._stream()), self.lib)

    def step_counts(self, dev_batch, n_pos, stride, denom, sampler_shaped=False, pack=0):
        """TransE sign-count step in one call: forward_counts + apply_counts with the middle fused on the device
        (include/kge_mi355.h kge_transe_train_step_counts; distribute_training.py:95-101,282).  Same bits as the two calls."""
        lr = float(self._adam_lr_t()) if self._adam else float(self.alpha)
        _lib.check(self.lib.kge_transe_train_step_counts_packed(
            ctypes.byref(self._desc), self._tab_ptrs, self._adam_m_ptrs if self._adam else None, self._adam_v_ptrs if self._adam else None,
            dev_batch[0].data_ptr(), dev_batch[1].data_ptr(), dev_batch[2].data_ptr(), (pack if sampler_shaped else 0) or None, n_pos,
            self.negative_ent + self.negative_rel,
            stride, denom, self._counts.data_ptr(), self._grad_ptrs, 1 if sampler_shaped else 0, 1 if self._adam else 0, lr,
            self.adam_beta1, self.adam_beta2, self.adam_epsilon, self._loss.data_ptr(), self._stream()), self.lib)
        if self._adam:
            self._adam_advance()
        self.global_step += 1

    def apply_counts(self, denom, own=False, piece=0):
        """Normalise-backward on the summed counts + SGD / TF1 Adam, both tables in one launch
        (distribute_training.py:95-101).  own=True (data-parallel): this rank's rows of the [(E+R), D] row space only,
        from its reduce-scattered chunk of the count image."""
        st = self._stream()
        lr = float(self._adam_lr_t()) if self._adam else float(self.alpha)
        m_ptrs = self._adam_m_ptrs if self._adam else None
        v_ptrs = self._adam_v_ptrs if self._adam else None
        if own:       # one piece of this rank's rows (the exchange loop advances Adam and the step counter once per step)
            row_lo, row_hi = self._piece_rows[piece]
            if row_hi > row_lo:
                img = self._counts_own.data_ptr() + 4 * piece * self._own_rows_len * self.hidden_size
                _lib.check(self.lib.kge_transe_apply_counts_range(
                    ctypes.byref(self._desc), self._tab_ptrs, m_ptrs, v_ptrs, img, self._grad_ptrs,
                    row_lo, row_hi, denom, 1 if self._adam else 0, lr, self.adam_beta1, self.adam_beta2,
                    self.adam_epsilon, st), self.lib)
            self._opt_state_synced = not self._adam
            return
        else:
            _lib.check(self.lib.kge_transe_apply_counts_tables(
                ctypes.byref(self._desc), self._tab_ptrs, m_ptrs, v_ptrs, self._counts.data_ptr(), self._grad_ptrs, denom,
                1 if self._adam else 0, lr, self.adam_beta1, self.adam_beta2, self.adam_epsilon, st), self.lib)
        if self._adam:
            self._adam_advance()
        self.global_step += 1

    def _check_ids(self, host):
        """Caller-supplied ids index device tables directly: an id out of range must fail here, not fault on the GPU."""
        if host.shape[1] == 0:
            return
        if host.min() < 0 or host[:2].max() >= self.entTotal or host[2].max() >= self.relTotal:
            raise KgeError("entity / relation id out of range in the supplied batch")

    def test_step(self, test_h, test_t, test_r):
        '''
        Score triples with the model's predict op (Config.py:478-488)
        On an entity table sharded across ranks this is a collective (every rank calls it, each with its own triples, possibly
        none): the rows of the triples' entities are fetched from their owners and scored as a compact table, with the bits of
        the single-process call.
        '''
        import torch
        host = np.stack([np.asarray(test_h), np.asarray(test_t), np.asarray(test_r)]).astype(np.int32)
        self._check_ids(host)
        if self._sharded("ent_embeddings"):
            return shard_eval.test_step(self, host)
        dev = torch.from_numpy(host).to(self.device)
        out = torch.empty(host.shape[1], dtype=torch.float32, device=self.device)
        self._predict(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), host.shape[1], out.data_ptr())
        self.trainModel.predict = out
        return out.cpu().numpy()

    # ------------------------------------------------------------------------------------------
    # triple classification and the predict_* helpers (Config.py:83-151, 491-516, 574-663)
    # ------------------------------------------------------------------------------------------
    def _tc_buffers(self, prefix, n):
        for side in ("pos", "neg"):
            for col in ("h", "t", "r"):
                arr = np.zeros(n, dtype=np.int64)
                setattr(self, "%s_%s_%s" % (prefix, side, col), arr)
                setattr(self, "%s_%s_%s_addr" % (prefix, side, col), arr.ctypes.data)

    def init_valid_triple_classification(self):
        """Evaluation files + the buffers getValidBatch / getBestThreshold fill (Config.py:123-151)."""
        if not getattr(self, "_eval_from_arrays", False):      # (an import by arrays stands: there are no files to read again)
            derived = getattr(self, "_type_lists_from", None) == "derived"
            self.lib.kge_clear_error()
            self.lib.importTestFiles()
            self._forget_evaluation()
            if derived:      # the lists were derived from the triples, not read: derive them from the new import too
                self.derive_type_constraints()
            else:
                self.lib.importTypeFiles()
            _lib.raise_if_error(self.lib)
        self.testTotal = self.lib.getTestTotal()
        self.validTotal = self.lib.getValidTotal()
        self._tc_buffers("valid", self.validTotal)
        self.relThresh = np.zeros(self.lib.getRelationTotal(), dtype=np.float32)
        self.relThresh_addr = self.relThresh.ctypes.data
        self.acc = np.zeros(1, dtype=np.float32)
        self.acc_addr = self.acc.ctypes.data

    def init_triple_classification(self):
        """The same plus the test-set buffers (Config.py:83-120)."""
        self.init_valid_triple_classification()
        self._tc_buffers("test", self.testTotal)

    def _alloc_tc_buffers(self):
        """init_triple_classification's buffers for an evaluation import that stands (init_evaluation_from_arrays)."""
        self.init_triple_classification()

    def _fit_thresholds(self):
        """Per-relation thresholds from the validation positives and their type-constrained negatives."""
        L = self.lib
        L.getValidBatch(self.valid_pos_h_addr, self.valid_pos_t_addr, self.valid_pos_r_addr,
                        self.valid_neg_h_addr, self.valid_neg_t_addr, self.valid_neg_r_addr)
        _lib.raise_if_error(L)
        res_pos = np.ascontiguousarray(self.test_step(self.valid_pos_h, self.valid_pos_t, self.valid_pos_r).reshape(-1), dtype=np.float32)
        res_neg = np.ascontiguousarray(self.test_step(self.valid_neg_h, self.valid_neg_t, self.valid_neg_r).reshape(-1), dtype=np.float32)
        L.getBestThreshold(self.relThresh_addr, res_pos.ctypes.data, res_neg.ctypes.data)

    def _test_triple_classification_host(self):
        """The host path (Config.py:491-503): thresholds from the validation scores, then the reference's routine on the test
        scores, which prints its four lines and gives the accuracy."""
        if not hasattr(self, "test_pos_h"):
            self.init_triple_classification()
        L = self.lib
        self._fit_thresholds()
        L.getTestBatch(self.test_pos_h_addr, self.test_pos_t_addr, self.test_pos_r_addr,
                       self.test_neg_h_addr, self.test_neg_t_addr, self.test_neg_r_addr)
        res_pos = np.ascontiguousarray(self.test_step(self.test_pos_h, self.test_pos_t, self.test_pos_r).reshape(-1), dtype=np.float32)
        res_neg = np.ascontiguousarray(self.test_step(self.test_neg_h, self.test_neg_t, self.test_neg_r).reshape(-1), dtype=np.float32)
        L.test_triple_classification(self.relThresh_addr, res_pos.ctypes.data, res_neg.ctypes.data, self.acc_addr)
        _lib.raise_if_error(L)
        return float(self.acc[0])

    def test(self):
        """Triple classification on the test set with thresholds fitted on the validation set, and / or link prediction,
        as the flags say (Config.py:491-516).  Returns a dict: {"acc": ..} and / or the link-prediction metrics."""
        import time
        t0 = time.time()
        result = {}
        if self.test_triple_classification:
            result["acc"] = self._test_triple_classification_host()
        if self.test_link_prediction:
            result.update(self.link_prediction()[1])
        if self.test_relation_prediction:
            result.update(self.relation_prediction()[1])
        print("\nElapsed test time (seconds): {}".format(time.time() - t0))
        return result

    # ---- triple classification on the device (csrc/tclass.hip) ----
    def _tc_upload(self, cols):
        """Six int64 id arrays (positives h, t, r; negatives h, t, r) -> one int32 device tensor [6, n], checked like test_step's."""
        import torch
        host = np.stack([np.asarray(c) for c in cols]).astype(np.int32)
        self._check_ids(host[:3])
        self._check_ids(host[3:])
        return torch.from_numpy(host).to(self.device)

    def _tc_scores(self, ids):
        """kge_predict over the positives and over the negatives of an uploaded batch, each in ONE call of the whole length as
        test_step makes it (the same arguments, so the same score bits) -> (pos, neg) device tensors."""
        import torch
        n = ids.shape[1]
        out = torch.empty((2, n), dtype=torch.float32, device=self.device)
        for side in range(2):
            self._predict(ids[3 * side].data_ptr(), ids[3 * side + 1].data_ptr(), ids[3 * side + 2].data_ptr(), n, out[side].data_ptr())
        return out

    def _tc_result_buffer(self):
        """One device allocation read back in one copy: int64 TP, TN, FP, FN followed by the fp32 thresholds."""
        import torch
        if getattr(self, "_tc_buf", None) is None or self._tc_buf.numel() != 32 + 4 * self.relTotal:
            self._tc_buf = torch.zeros(32 + 4 * self.relTotal, dtype=torch.uint8, device=self.device)
        return self._tc_buf, self._tc_buf[:32].view(torch.int64), self._tc_buf[32:].view(torch.float32)

    def _tc_fit_apply(self, valid_ids, split_ids, split):
        """predict -> kge_tc_fit -> (predict) -> kge_tc_apply on the current stream; the device thresholds and counts."""
        buf, counts, thresh = self._tc_result_buffer()
        st = self._stream()
        v = self._tc_scores(valid_ids)
        n_valid = valid_ids.shape[1]
        _lib.check(self.lib.kge_tc_fit(v[0].data_ptr(), v[1].data_ptr(), n_valid, thresh.data_ptr(), None, st), self.lib)
        s = v if split_ids is valid_ids else self._tc_scores(split_ids)
        _lib.check(self.lib.kge_tc_apply(split, thresh.data_ptr(), s[0].data_ptr(), s[1].data_ptr(), split_ids.shape[1],
                                         counts.data_ptr(), None, st), self.lib)
        return buf

    def _validation_accuracy_host(self, valid):
        ph, pt, pr, nh, nt, nr = valid
        pos = np.ascontiguousarray(self.test_step(ph, pt, pr).reshape(-1), dtype=np.float32)
        neg = np.ascontiguousarray(self.test_step(nh, nt, nr).reshape(-1), dtype=np.float32)
        thresh = np.zeros(self.relTotal, np.float32)
        self.lib.getBestThreshold(thresh.ctypes.data, pos.ctypes.data, neg.ctypes.data)
        correct = (pos <= thresh[pr]).sum() + (neg > thresh[nr]).sum()
        return float(correct) / (2.0 * max(len(pos), 1))

    def validation_accuracy(self, valid=None):
        """The early-stop check's accuracy (distribute_training.py:295-333): thresholds fitted on the validation triples and
        their negatives, then the share of those 2 V answers the thresholds get right -- correct / (2 V), the Python float the
        host formula gives.  `valid` = the six id arrays getValidBatch filled (positives h, t, r; negatives h, t, r); None draws
        them with getValidBatch on the first call.  The ids go to the device once and stay there for as long as the same
        list object is passed -- its arrays must not be refilled in place (pass a new list for a new batch); scores, thresholds and counts never leave it, and only the four counts are read back.
        On an entity table sharded across ranks this is the host path (test_step is a collective there): the scores come to
        the host and getBestThreshold runs on them, as before."""
        if valid is None:
            valid = getattr(self, "_tc_valid_drawn", None)
            if valid is None:
                if not hasattr(self, "valid_pos_h"):
                    self.init_valid_triple_classification()
                self.lib.getValidBatch(self.valid_pos_h_addr, self.valid_pos_t_addr, self.valid_pos_r_addr,
                                       self.valid_neg_h_addr, self.valid_neg_t_addr, self.valid_neg_r_addr)
                _lib.raise_if_error(self.lib)
                # copies: test() and triple_classification() draw new negatives into the same buffers
                valid = self._tc_valid_drawn = [a.copy() for a in (self.valid_pos_h, self.valid_pos_t, self.valid_pos_r,
                                                                   self.valid_neg_h, self.valid_neg_t, self.valid_neg_r)]
        if self._sharded("ent_embeddings"):
            return self._validation_accuracy_host(valid)
        cached = getattr(self, "_tc_valid_dev", None)
        if cached is None or cached[0] is not valid:
            cached = self._tc_valid_dev = (valid, self._tc_upload(valid))
        ids = cached[1]
        if ids.shape[1] == 0:
            return 0.0
        counts = self._tc_fit_apply(ids, ids, 0)[:32].cpu().numpy().view(np.int64)
        return float(int(counts[0]) + int(counts[1])) / (2.0 * max(ids.shape[1], 1))

    def _tc_draw(self, split):
        """The batches of a device classification call, drawn exactly as test() draws them (getValidBatch, then for "test"
        getTestBatch) and uploaded once -> (valid ids, split ids), the same tensor for "valid"."""
        if not hasattr(self, "test_pos_h"):
            self.init_triple_classification()
        L = self.lib
        L.getValidBatch(self.valid_pos_h_addr, self.valid_pos_t_addr, self.valid_pos_r_addr,
                        self.valid_neg_h_addr, self.valid_neg_t_addr, self.valid_neg_r_addr)
        valid = [self.valid_pos_h, self.valid_pos_t, self.valid_pos_r, self.valid_neg_h, self.valid_neg_t, self.valid_neg_r]
        batch = valid
        if split == "test":
            L.getTestBatch(self.test_pos_h_addr, self.test_pos_t_addr, self.test_pos_r_addr,
                           self.test_neg_h_addr, self.test_neg_t_addr, self.test_neg_r_addr)
            batch = [self.test_pos_h, self.test_pos_t, self.test_pos_r, self.test_neg_h, self.test_neg_t, self.test_neg_r]
        _lib.raise_if_error(L)
        valid_ids = self._tc_upload(valid)      # new negatives every call: nothing to keep beyond it
        return valid_ids, (self._tc_upload(batch) if split == "test" else valid_ids)

    def triple_classification(self, split="test"):
        """Triple classification of a split ("test" or "valid") with thresholds fitted on the validation set, on the device:
        {"acc", "precision", "recall", "f1", "tp", "tn", "fp", "fn"}.  The batches are drawn on the host exactly as test() draws
        them (getValidBatch, then for "test" getTestBatch: the same libc rand() draws, the same negatives), uploaded once per call as
        int32; kge_predict, kge_tc_fit and kge_tc_apply then run on one stream and a single copy brings back the four
        counts and the thresholds, which fill self.relThresh for predict_triple.  "acc" is the float32 test() returns.
        On an entity table sharded across ranks this is test()'s host path unchanged (test_step is a collective there): the
        test split only, and the result holds "acc" alone, which is all the host routine returns."""
        if split not in ("test", "valid"):
            raise KgeError("triple_classification: split must be 'test' or 'valid'")
        if self._sharded("ent_embeddings"):
            if split != "test":
                raise KgeError("triple_classification over an entity table sharded across ranks: the host path classifies the test split only")
            return {"acc": self._test_triple_classification_host()}
        import torch
        valid_ids, split_ids = self._tc_draw(split)
        _, _, thresh = self._tc_result_buffer()
        thresh.copy_(torch.from_numpy(self.relThresh))     # relations without validation triples keep their value, as on the host
        host = self._tc_fit_apply(valid_ids, split_ids, 1 if split == "test" else 0).cpu().numpy()
        tp, tn, fp, fn = (int(x) for x in host[:32].view(np.int64))
        self.relThresh[:] = host[32:].view(np.float32)
        ratio = lambda a, b: a / b if b else float("nan")
        precision, recall = ratio(1.0 * tp, tp + fp), ratio(1.0 * tp, tp + fn)
        acc = ratio(1.0 * (tp + tn), tp + tn + fp + fn)
        return {"acc": float(np.float32(acc)), "precision": precision, "recall": recall,
                "f1": ratio(2 * precision * recall, precision + recall), "tp": tp, "tn": tn, "fp": fp, "fn": fn}

    # ---- ROC curves and AUC on the device (kge_tc_roc, csrc/tclass.hip) ----
    def _roc_device(self, split, rel_index=None):
        """Draw and score as triple_classification(split) does, then kge_tc_roc for every relation at once ->
        (auc2 [R, 2] int64 on the host, curve).  With rel_index a first call with an empty count buffer only reports the
        sizes (it ends behind its wait, before any binning), a second fills a buffer of that size, and curve = (that
        relation's get_TPFP counts, its n_interval, the minimum of its validation scores); without it curve is None and
        only the [R][2] buffer is read back."""
        import torch
        if split not in ("test", "valid"):
            raise KgeError("roc: split must be 'test' or 'valid'")
        if self._sharded("ent_embeddings"):
            raise KgeError("ROC curves over an entity table sharded across ranks would fetch the rows of every validation and "
                           "test triple to one rank: triple_classification (the host path, a collective there) is what sharded tables have")
        R = self.relTotal
        if rel_index is not None and not 0 <= rel_index < R:      # before the draw: a refused call consumes no rand()
            raise KgeError("roc_curve: relation %r out of range" % (rel_index,))
        valid_ids, split_ids = self._tc_draw(split)
        st = self._stream()
        v = self._tc_scores(valid_ids)
        s = v if split_ids is valid_ids else self._tc_scores(split_ids)
        auc2 = torch.empty((R, 2), dtype=torch.int64, device=self.device)
        offsets = np.zeros(R + 1, dtype=np.int64)

        def call(tpfp, capacity):
            return self.lib.kge_tc_roc(v[0].data_ptr(), v[1].data_ptr(), valid_ids.shape[1], 1 if split == "test" else 0,
                                       s[0].data_ptr(), s[1].data_ptr(), split_ids.shape[1], auc2.data_ptr(),
                                       tpfp.data_ptr() if tpfp is not None else None, capacity, offsets.ctypes.data, st)
        if rel_index is None:
            _lib.check(call(None, 0), self.lib)
            return auc2.cpu().numpy(), None
        # sizes first: a count buffer declared empty makes the call stop behind its one wait, h_offsets filled and nothing
        # binned or written (a relation without validation triples is then refused before any binning too)
        offsets[R] = -1
        tpfp = torch.empty(1, dtype=torch.int64, device=self.device)
        rc = call(tpfp, 0)
        if offsets[R] < 0:
            _lib.check(rc, self.lib)      # another error: its own message
        self.lib.kge_clear_error()
        lo, hi = int(offsets[rel_index]), int(offsets[rel_index + 1])
        if hi == lo:
            raise KgeError("roc_curve: relation %d has no validation triples, so no threshold grid" % rel_index)
        tpfp = torch.empty(int(offsets[R]), dtype=torch.int64, device=self.device)
        _lib.check(call(tpfp, tpfp.numel()), self.lib)
        mask = valid_ids[2] == rel_index
        mn = torch.minimum(v[0][mask].min(), v[1][mask].min()).cpu().numpy() + np.float32(0.0)      # -0 -> +0, as the kernel
        return auc2.cpu().numpy(), (tpfp[lo:hi].cpu().numpy(), (hi - lo) // 2 - 1, np.float32(mn))

    @staticmethod
    def _grid_points(mn, n_interval):
        """g(i) = fmaf((float)i, 0.01f, mn), i = 0..n_interval, with ONE rounding as the library forms it: the product is exact
        in double, the sum is rounded to odd there (TwoSum gives its exact error), so the rounding to float32 is the correct one."""
        p = np.arange(n_interval + 1, dtype=np.float64) * np.float64(np.float32(0.01))
        b = np.float64(mn)
        s = p + b
        bb = s - p
        err = (p - (s - bb)) + (b - bb)
        even = (s.view(np.int64) & 1) == 0
        s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)

    def roc_auc(self, split="test"):
        """Area under every relation's ROC curve on a split ("test" or "valid"), on the device: {"auc": float64 [relTotal],
        NaN for a relation without validation or without split triples, "n": int64 [relTotal] the relation's triples in the
        split, "macro": the mean of the defined values, "weighted": sum n_r auc_r / sum n_r}.  The curve of relation r is
        get_TPFP's: the split's positives (TP) and negatives (FP) at or below each point of the grid the validation scores span,
        closed by (0, 0) and (n_r, n_r); auc_r = area2 / (2 n_r^2), one Python-float division of the exact integers kge_tc_roc
        returns.  The batches are drawn exactly as triple_classification(split) draws them (the same libc rand() draws, the same
        negatives), uploaded once, scored by one kge_predict per side, and one [relTotal][2] buffer is read back.
        Raises KgeError on an entity table sharded across ranks."""
        auc2, _ = self._roc_device(split)
        n = auc2[:, 1].copy()
        auc = np.array([int(a) / (2 * int(k) * int(k)) if k else float("nan") for a, k in auc2], dtype=np.float64).reshape(-1)
        have = n > 0
        macro = float(auc[have].mean()) if have.any() else float("nan")
        weighted = float((n[have] * auc[have]).sum() / n[have].sum()) if have.any() else float("nan")
        return {"auc": auc, "n": n, "macro": macro, "weighted": weighted}

    def roc_curve(self, rel_index, split="test"):
        """The ROC curve of one relation on a split: {"tp", "fp": int64 [n_interval + 1], get_TPFP's counts at every grid
        point, "thresholds": the float32 grid points fmaf(i, 0.01f, min), "tpr", "fpr": the counts over the relation's OWN
        number of split triples n_r (NaN when it has none), "auc": as roc_auc's, "n": n_r}.  Draws and scores as roc_auc does.
        Raises KgeError for a relation without validation triples (where get_TPFP returns 0) and on a sharded entity table."""
        auc2, (counts, n_interval, mn) = self._roc_device(split, int(rel_index))
        tp, fp = counts[:n_interval + 1].copy(), counts[n_interval + 1:].copy()
        area2, n_r = int(auc2[rel_index, 0]), int(auc2[rel_index, 1])
        nan = float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            tpr, fpr = (tp / np.float64(n_r), fp / np.float64(n_r)) if n_r else (np.full(len(tp), nan), np.full(len(fp), nan))
        return {"tp": tp, "fp": fp, "thresholds": self._grid_points(mn, n_interval), "tpr": tpr, "fpr": fpr,
                "auc": area2 / (2 * n_r * n_r) if n_r else nan, "n": n_r}

    @staticmethod
    def _roc_lists(counts, n_interval, total):
        """The reference's TPR / FPR lists and area (Config.py:536-556) from get_TPFP's counts (TP(0..n) then FP(0..n)) ->
        (TPR, FPR, auc): a (0, 0) start point unless the first grid point already counts nothing, the counts, an end point
        (total, total) unless the last grid point already counts the whole list, every element divided by the last, np.trapz."""
        res = [int(c) for c in counts]
        TPR, FPR = [], []
        if res[0] != 0 or res[0 + n_interval + 1] != 0:
            TPR.append(0)
            FPR.append(0)
        for i in range(0, n_interval + 1):
            TPR.append(res[i])
            FPR.append(res[i + n_interval + 1])
        if TPR[len(TPR) - 1] != total or FPR[len(FPR) - 1] != total:
            TPR.append(total)
            FPR.append(total)
        for i in range(len(TPR)):
            TPR[i] /= TPR[-1]
        for i in range(len(FPR)):
            FPR[i] /= FPR[-1]
        trapz = getattr(np, "trapezoid", None) or np.trapz      # one function under two names across NumPy versions
        return TPR, FPR, trapz(TPR, FPR)

    def plot_roc(self, rel_index, fig_name=None):
        """The reference's plot_roc (Config.py:519-571): the ROC curve of one relation on the test split, drawn with the
        reference's labels and shown, or saved when fig_name is given; returns (FPR, TPR, auc) as plotted.  The lists are
        built literally as the reference builds them (_roc_lists), whose end point is the length of the WHOLE test list: it is
        the relation's own count only for a one-relation test list, so on any other the plotted curve ends in a long closing
        segment and its area is not the relation's AUC.  roc_curve normalises by the relation's own count for that reason.
        The counts come from kge_tc_roc.  Raises KgeError as roc_curve does."""
        _, (counts, n_interval, _) = self._roc_device("test", int(rel_index))
        TPR, FPR, auc = self._roc_lists(counts, n_interval, len(self.test_pos_h))
        import matplotlib.pyplot as plt
        plt.figure()
        lw = 2
        plt.plot(FPR, TPR, color='darkorange', lw=lw, label='ROC curve (area = %0.3f)' % auc)
        plt.plot([0, 1], [0, 1], color='navy', lw=lw, linestyle='--')
        plt.xlim([0.0, 1.0])
        plt.ylim([0.0, 1.05])
        plt.xlabel('False Positive Rate (FPR)')
        plt.ylabel('True Positive Rate (TPR)')
        plt.title('ROC Curve')
        plt.legend(loc="lower right")
        if fig_name is None or fig_name == '':
            plt.show()
        else:
            plt.savefig(fig_name)
        return FPR, TPR, auc

    def _top_k(self, scores, k):
        res = np.asarray(scores).reshape(-1).argsort()[:k]
        print(res)
        return res

    def _refuse_sharded_predict(self, what):
        if self._sharded("ent_embeddings"):
            raise KgeError("%s over an entity table sharded across ranks would fetch every row to every rank: rank test triples with "
                           "link_prediction (a collective on sharded tables) instead" % what)

    def predict_head_entity(self, t, r, k):
        """The k head entities that score best for (?, t, r) (Config.py:574-593)."""
        self._refuse_sharded_predict("predict_head_entity")
        ar = np.arange(self.entTotal)
        return self._top_k(self.test_step(ar, np.full(self.entTotal, t), np.full(self.entTotal, r)), k)

    def predict_tail_entity(self, h, r, k):
        """The k tail entities that score best for (h, ?, r) (Config.py:595-614)."""
        self._refuse_sharded_predict("predict_tail_entity")
        ar = np.arange(self.entTotal)
        return self._top_k(self.test_step(np.full(self.entTotal, h), ar, np.full(self.entTotal, r)), k)

    def predict_relation(self, h, t, k):
        """The k relations that score best for (h, t, ?) (Config.py:616-635; TransR's predict op uses the matrix of
        the FIRST relation of a call, TransR.py:83, like the reference).
        Batched, filtered and type-constrained on the device, each TransR relation with its own matrix: top_k_relations."""
        ar = np.arange(self.relTotal)
        return self._top_k(self.test_step(np.full(self.relTotal, h), np.full(self.relTotal, t), ar), k)

    def predict_triple(self, h, t, r, thresh=None):
        """Is (h, t, r) correct?  Score below `thresh`, or below the relation's threshold fitted on the validation set
        (Config.py:637-663).  Prints the reference's message and also returns the verdict."""
        res = float(self.test_step(np.array([h]), np.array([t]), np.array([r])).reshape(-1)[0])
        if thresh is None:
            if not hasattr(self, "valid_pos_h"):
                self.init_triple_classification()
            self._fit_thresholds()
            thresh = float(self.relThresh[r])
        ok = res < thresh
        print("triple (%d,%d,%d) is %s" % (h, t, r, "correct" if ok else "wrong"))
        return ok

    # evaluation by ranking: these methods document the calls and dispatch to rank_eval ---------------------------
    def top_k_tails(self, h, r, k, filtered=False, type_constrained=False):
        """The k best tails of (h, r, ?) for every query, ranked on the device (kge_topk_entities).  h and r are ints or 1-D
        arrays, broadcast against each other.  Returns (ids int64 [n, k], scores float32 [n, k]) in ascending (score, id)
        order, padded with -1 / +inf where fewer than k candidates are eligible; numpy in gives numpy out, device tensors in
        give device tensors out.  filtered drops known triples (train + valid + test), type_constrained keeps the relation's
        tail type list -- both need init_link_prediction().  bf16 tables: set_bf16_evaluation chooses between a float32 view and
        the stored rows (kge_topk_entities_bf16), with the same ids and score bits.
        On an entity table sharded across ranks it is a collective: every rank calls it the same number of times, each with
        its own queries (possibly none) and the same k, side and flags, and gets the results of its own queries, with the bits
        of one process over the whole table (kge_topk_entities_range, kge_topk_merge_keys).  Arguments invalid on any rank,
        or k / side / flags differing between ranks, raise KgeError on every rank."""
        return rank_eval.top_k_entities(self, h, r, k, False, filtered, type_constrained)

    def top_k_heads(self, t, r, k, filtered=False, type_constrained=False):
        """The k best heads of (?, r, t) for every query; as top_k_tails."""
        return rank_eval.top_k_entities(self, t, r, k, True, filtered, type_constrained)

    def top_k_relations(self, h, t, k, filtered=False, type_constrained=False):
        """The k best relations of (h, ?, t) for every query, scored and selected on the device (kge_topk_relations).  h and t
        are ints or 1-D arrays, broadcast against each other.  Returns (ids int64 [n, k], scores float32 [n, k]) in ascending
        (score, id) order, padded with -1 / +inf where fewer than k relations are eligible; numpy in gives numpy out, device
        tensors in give device tensors out.  Scores are kge_predict's, TransR with each relation's own matrix.  filtered drops
        relations forming a known triple (train + valid + test), type_constrained keeps relations whose head / tail type lists
        hold h / t -- both need init_link_prediction()."""
        return rank_eval.top_k_relations(self, h, t, k, filtered, type_constrained)

    def link_prediction_distributed(self, test_head=True):
        """The whole test set, split into one contiguous range per rank (the static split of
        distribute_training.py:430-441) and reduced like main_spark.py:430-448: every rank returns the global metrics.
        On a sharded entity table the candidates are split instead: link_prediction over the whole test set, a collective."""
        return rank_eval.link_prediction_distributed(self, test_head)

    def link_prediction(self, first=0, count=None, test_head=True):
        """Rank every test triple in [first, first+count) on the device (replaces the per-triple loop of
        distribute_training.py:465-590).  Returns (raw int64 [count,2,8] as testTail/testHead give them,
        metrics dict with the reference's accumulator names normalised by the number of triples, the way
        main_spark.py:430-448 reduces them: r_* = tail prediction, l_* = head prediction).
        On an entity table sharded across ranks it is a collective (every rank calls it with the same arguments and gets the same
        result): each rank ranks the triples against its own rows (kge_link_prediction_range) and the counts and arg-mins are merged
        across ranks.  Its scores may place a near-tie (a candidate within an ulp or so of the true triple) on the other side of
        the true triple than kge_link_prediction does."""
        return rank_eval.link_prediction(self, first, count, test_head)

    def _refuse_sharded_rank(self, what):
        if self._sharded("ent_embeddings"):
            raise KgeError("%s over an entity table sharded across ranks is not supported: call the collective "
                           "%s_distributed on every rank (or rank the test triples with link_prediction, a collective on "
                           "sharded tables)" % (what, what))

    def rank_triples(self, h, t, r, test_head=True):
        """Rank any triples on the device (kge_rank_triples): h, t, r are 1-D id arrays of one length, in any order, with any
        mix of relations and with duplicates -- the validation split, or triples of the caller's own.  Returns (counts int64
        [n, 2, 4], metrics): counts[i, 0] ranks every entity as the tail of (h, r, ?), counts[i, 1] as the head of (?, r, t)
        (zeros with test_head=False); the columns are the numbers of candidates other than the target that score strictly below
        the true triple -- raw, filtered (train + valid + test), typed, filtered + typed -- exactly columns 0..3 of
        link_prediction's rows, from the same score bits.  metrics has link_prediction's names, normalised by n.  Needs
        init_link_prediction().  An id out of range raises KgeError before anything is launched.  bf16 tables:
        set_bf16_evaluation chooses between a float32 view and the stored rows (kge_rank_triples_bf16), with the same counts."""
        return rank_eval.rank_triples(self, h, t, r, test_head)

    def rank_triples_distributed(self, h, t, r, test_head=True):
        """rank_triples as a collective: every rank passes the same triples and gets the same (counts int64 [n, 2, 4],
        metrics), with rank_triples's column meaning and metric names.  Arguments invalid on any rank (an id out of range is
        found before anything is launched), or n / test_head differing between ranks, raise KgeError on every rank and leave
        none waiting.
        On an entity table sharded across ranks (TransE) every rank ranks the triples against its own rows
        (kge_rank_triples_range), in rounds of lp_shard_query_bytes // (2 D 4) triples whose h and t rows come from their
        owners, and one SUM all-reduce merges the counts: bit for bit those of one process over the whole table with the same
        kernel, for any number of ranks.  Its scores are link_prediction's on a sharded table: a candidate within an ulp or so
        of the true triple may fall on the other side of it than kge_rank_triples (rank_triples) puts it.
        On replicated tables (all four models) rank g ranks the g-th contiguous slice of the triples with kge_rank_triples and
        one SUM all-reduce merges the slices: exactly rank_triples's counts.  With one process and no process group it is
        rank_triples."""
        if not self._sharded("ent_embeddings") and self.world_size <= 1:
            return self.rank_triples(h, t, r, test_head)
        return rank_eval.rank_ids_distributed(self, lambda: rank_eval.triple_ids(self, h, t, r), test_head)

    # candidate lists instead of every entity (kge_rank_candidates) ------------------------------------------------------------
    def _refuse_sharded_candidates(self, what):
        if self._sharded("ent_embeddings"):
            raise KgeError("%s over an entity table sharded across ranks is not supported: call one of the collectives "
                           "rank_candidates_distributed, rank_triples_sampled_distributed or "
                           "validation_link_prediction_distributed(candidates=C) on every rank" % what)

    def rank_candidates(self, h, t, r, tail_candidates=None, head_candidates=None, filtered=True):
        """Rank triples against candidate lists of the caller's instead of every entity (kge_rank_candidates): h, t, r are 1-D id
        arrays of one length n; a candidate array is [n, C] (one list per triple) or [C] (one list shared by all), integer, as
        numpy or as a torch tensor (a device tensor is not copied to the host).  An id outside [0, entTotal) is skipped, so -1
        pads ragged lists; a repeated id counts every time.  Both lists must have the same C when both are given; a side
        without a list is not ranked.  Returns (counts int64 [n, 2, 2], metrics): counts[i, 0] ranks the tail list of (h, r, ?),
        counts[i, 1] the head list of (?, r, t); column 0 is the number of listed candidates other than the target that score
        strictly below the true triple, column 1 the same without the candidates forming a known triple (train + valid + test;
        needs init_link_prediction() -- with filtered=False it is not computed, equals column 0 and nothing is needed).  metrics
        has link_prediction's raw and _filter names for the ranked sides, normalised by n.  The scores are test_step's bits.
        An id of a TRIPLE out of range raises KgeError before anything is launched."""
        return rank_eval.rank_candidates(self, h, t, r, tail_candidates, head_candidates, filtered)

    def rank_candidates_distributed(self, h, t, r, tail_candidates=None, head_candidates=None, filtered=True):
        """rank_candidates as a collective: every rank passes the same arguments and gets the same (counts int64 [n, 2, 2],
        metrics).  Invalid arguments on any rank, or arguments differing between ranks, raise KgeError on every rank.
        On an entity table sharded across ranks (TransE) every rank ranks the triples against the listed candidates whose rows it
        owns (kge_rank_candidates_range), in rounds of lp_shard_query_bytes // (2 D 4) triples whose h and t rows come from their
        owners, and one SUM all-reduce merges the counts: bit for bit rank_candidates' counts over the whole table.
        On replicated tables rank g ranks the g-th contiguous slice of the triples and one SUM all-reduce merges the slices.
        With one process and no process group it is rank_candidates."""
        if not rank_eval.sharded_in_group(self, "rank_candidates_distributed") and self.world_size <= 1:
            return self.rank_candidates(h, t, r, tail_candidates, head_candidates, filtered)
        return rank_eval.rank_candidates_distributed(self, h, t, r, tail_candidates, head_candidates, filtered)

    def rank_triples_sampled(self, h, t, r, n_candidates, seed=0, test_head=True, type_constrained=False, filtered=True):
        """rank_candidates against n_candidates entities per (triple, side) that the device draws from a counter hash of (seed,
        triple index, side, position) -- sampled_candidates returns the very ids -- so no list exists in memory.  With
        type_constrained=True they come from the relation's tail / head type list (a relation without one: from all entities;
        needs the type lists).  test_head=False ranks the tail side only.  Returns (counts int64 [n, 2, 2], metrics) as
        rank_candidates does; the same seed gives the same lists on every call."""
        return rank_eval.rank_triples_sampled(self, h, t, r, n_candidates, seed, test_head, type_constrained, filtered)

    def rank_triples_sampled_distributed(self, h, t, r, n_candidates, seed=0, test_head=True, type_constrained=False, filtered=True):
        """rank_triples_sampled as a collective: every rank passes the same arguments.  On replicated tables rank g ranks the g-th
        contiguous slice of the triples and one SUM all-reduce merges the slices.  On an entity table sharded across ranks
        (TransE) every rank draws every list and ranks the candidates whose rows it owns (kge_rank_candidates_range), as
        rank_candidates_distributed does.  The hash is indexed by the global triple index,
        so the counts are those of one process.  Invalid arguments on any rank, or arguments differing between ranks, raise
        KgeError on every rank.  With one process and no process group it is rank_triples_sampled."""
        what = "rank_triples_sampled_distributed"
        if not rank_eval.sharded_in_group(self, what) and self.world_size <= 1:
            return self.rank_triples_sampled(h, t, r, n_candidates, seed, test_head, type_constrained, filtered)
        triples = lambda: rank_eval.triple_ids(self, h, t, r)
        return rank_eval.rank_sampled_distributed(self, what, triples, n_candidates, seed, test_head, type_constrained, filtered)

    def sampled_candidates(self, n, n_candidates, seed, side, r=None, type_constrained=False):
        """The ids rank_triples_sampled draws for `side` (0: tail lists, 1: head lists) of triples 0 .. n-1, restated in numpy:
        int64 [n, n_candidates].  With type_constrained=True `r` (the n relation ids) is needed: the ids come from the engine's
        tail / head type list of each triple's relation (type_constraints()), from all entities where that list is empty."""
        if side not in (0, 1):
            raise KgeError("sampled_candidates: side must be 0 (tail) or 1 (head)")
        i = np.arange(int(n), dtype=np.int64)[:, None]
        k = np.arange(int(n_candidates), dtype=np.int64)[None, :]
        ids = _lib.drawn_candidate_index(seed, i, side, k, self.entTotal)
        if type_constrained:
            if r is None:
                raise KgeError("sampled_candidates: type_constrained=True needs the triples' relation ids")
            r = np.asarray(r, dtype=np.int64).reshape(-1)
            if len(r) != int(n):
                raise KgeError("sampled_candidates: r must hold n = %d relation ids" % int(n))
            head_off, head_ids, tail_off, tail_ids = self.type_constraints()
            off, lst = (head_off, head_ids) if side else (tail_off, tail_ids)
            lo, length = off[r][:, None], (off[r + 1] - off[r])[:, None]
            typed = _lib.drawn_candidate_index(seed, i, side, k, np.maximum(length, 1))
            ids = np.where(length > 0, lst[np.minimum(lo + typed, max(len(lst) - 1, 0))] if len(lst) else ids, ids)
        return ids

    def validation_link_prediction(self, test_head=True, sample=0, candidates=0, seed=0, type_constrained=False):
        """rank_triples on the positives of valid2id.txt (read from in_path in file order; getValidBatch is not used, so the
        libc rand() sequence does not move): (counts, metrics) as rank_triples returns them -- filtered Hits@10 and MRR on the
        validation split for model selection.  sample = N > 0 ranks the N triples at the indices floor(i V / N), i < N (all
        of them when N >= V); one check scores V x E pairs per side otherwise.  The device ids are kept between calls.
        candidates = C > 0 ranks the chosen triples against C drawn candidates per side instead of every entity
        (rank_triples_sampled with `seed`, from the type lists with type_constrained=True): (counts int64 [n, 2, 2], metrics) as
        rank_triples_sampled returns them, V x C pairs per side."""
        return rank_eval.validation_link_prediction(self, test_head, sample, candidates, seed, type_constrained)

    def validation_link_prediction_distributed(self, test_head=True, sample=0, candidates=0, seed=0, type_constrained=False):
        """validation_link_prediction as a collective, ranked as rank_triples_distributed ranks (sharded or replicated
        tables; its near-tie caveat on a sharded table applies): the same valid2id.txt positives, the same `sample` rule and
        the same cached device ids; every rank calls it with the same arguments and gets the same (counts, metrics).  A bad
        `sample` or an unreadable valid2id.txt on any rank raises KgeError on every rank.
        candidates = C > 0 ranks against C drawn candidates per side as validation_link_prediction(candidates=C) does, with
        rank_triples_sampled_distributed's split (sharded: every rank counts the candidates it owns; replicated: slices of the
        triples): (counts int64 [n, 2, 2], metrics), exactly one process's counts.  A bad value on any rank raises on every rank."""
        if not self._sharded("ent_embeddings") and self.world_size <= 1:
            return self.validation_link_prediction(test_head, sample, candidates, seed, type_constrained)
        return rank_eval.validation_link_prediction_distributed(self, test_head, sample, candidates, seed, type_constrained)

    def relation_prediction(self, first=0, count=None):
        """Rank the true relation of every test triple in [first, first+count) (kge_link_prediction's order) among all
        relations on the device (kge_relation_prediction).  Returns (raw int64 [count, 4]: the relations scoring strictly
        better, raw / filtered / typed / filtered + typed, and the 20 rel* metrics normalised by the number of triples).
        Without type_constrain.txt the typed columns are 0.
        On an entity table sharded across ranks it is a collective: every rank calls it with the same arguments and gets the
        same result, bit for bit that of one process over the whole table.  Each rank ranks one contiguous slice of the
        triples from h / t rows fetched from their owners (kge_relation_prediction_rows) and the counts are summed across
        ranks.  Arguments invalid on any rank, or first / count differing between ranks, raise KgeError on every rank."""
        return rank_eval.relation_prediction(self, first, count)

    def relation_prediction_distributed(self):
        """relation_prediction over the whole test set split into one contiguous range per rank and all-reduced, as
        link_prediction_distributed does: every rank returns the global metrics.
        On a sharded entity table it is relation_prediction over the whole test set, a collective."""
        return rank_eval.relation_prediction_distributed(self)

    # ------------------------------------------------------------------------------------------
    # parameters by the reference's variable names (Config.py:378-421)
    # ------------------------------------------------------------------------------------------
    def get_parameter_lists(self):
        return self.trainModel.parameter_lists

    def _sharded(self, var_name):
        return self._dp and getattr(self, "sparse_rows", False) and var_name == "ent_embeddings" and hasattr(self, "_shard")

    def get_parameters_by_name(self, var_name):
        if var_name in self.trainModel.parameter_lists:
            t = self.trainModel.parameter_lists[var_name]
            if self._sharded(var_name):   # collective: every rank must call it (the shards are gathered; small tables only)
                import torch
                from .parallel import all_gather_chunks
                self.comm_fence("pg")
                full = torch.empty((self._shard["chunk"] * self.world_size, t.shape[1]), dtype=t.dtype, device=t.device)
                all_gather_chunks(full.view(-1), t.reshape(-1), self._pg)
                return full[:self.entTotal].cpu().numpy()
            if self._bf16:      # float32 out: an exact widening
                return t.detach().float().cpu().numpy()
            return t.detach().cpu().numpy()
        return None

    def get_parameters(self, mode="numpy"):
        res = {}
        for var_name in self.get_parameter_lists():
            if mode == "numpy":
                res[var_name] = self.get_parameters_by_name(var_name)
            else:
                res[var_name] = self.get_parameters_by_name(var_name).tolist()
        return res

    def save_parameters(self, path=None):
        if path == None:
            path = self.out_path
        with open(path, "w") as f:
            f.write(json.dumps(self.get_parameters("list")))

    def tables_changed(self):
        """Tell the engine that device tables were written from outside its kernels (it keeps a per-row 1/|row| table for
        the TransE emit kernel current across steps, include/kge_mi355.h "tables_changed").  Everything in this package that
        writes tables calls it; call it yourself after writing `parameter_lists[...]` tensors directly."""
        self.lib.kge_set_option(b"tables_changed", 1)

    def set_parameters_by_name(self, var_name, tensor):
        import torch
        if var_name in self.trainModel.parameter_lists:
            dst = self.trainModel.parameter_lists[var_name]
            src = torch.as_tensor(np.asarray(tensor, dtype=np.float32))
            if self._sharded(var_name):
                lo, hi = self._shard["lo"], self._shard["hi"]
                dst[:hi - lo].copy_(src.reshape(self.entTotal, -1)[lo:hi])
            else:
                dst.copy_(src.reshape(dst.shape))      # (bf16 tables: the copy rounds to nearest-even)
            self._drop_eval_view()
            self.tables_changed()

    def set_parameters(self, lists):
        for i in lists:
            self.set_parameters_by_name(i, lists[i])

    def get_gradients(self):
        """Current contents of the dense gradient accumulators (zero between steps)."""
        return {n: g.detach().cpu().numpy() for n, g in zip(self.trainModel.table_names, self._grads)}

    def get_stream_states(self, before_prefetch=False):
        """rng stream states of the virtual sampler threads (next_random[], Random.h:6).  With sampling one step ahead
        (prefetch_sampling) the device states are those AFTER the prefetched batch was drawn; before_prefetch=True rewinds
        them by that one batch (what a checkpoint must store so that a resumed run trains on the prefetched batch too)."""
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        out = np.zeros(self.workThreads, dtype=np.uint64)
        _lib.check(self.lib.kge_get_stream_states(out.ctypes.data, self.workThreads), self.lib)
        if before_prefetch and getattr(self, "_prefetched", None) is not None:
            from .parallel import slice_positions
            draws = 1 + 2 * self.negative_ent + self.negative_rel          # rng draws per positive (Base.cpp:101-139)
            for i in range(self.workThreads):
                _, cnt = slice_positions(self.batch_size, self.workThreads, i, i + 1)
                out[i] = np.uint64(lcg_jump(int(out[i]), -cnt * draws))
        return out


LCG_A, LCG_C, MASK64 = 25214903917, 11, (1 << 64) - 1   # Random.h:16-19: x = x * 25214903917 + 11 (mod 2^64)


def lcg_jump(state, n):
    """The stream state n draws later (n < 0: earlier; the generator has full period 2^64, so stepping back n draws is
    stepping forward 2^64 - n)."""
    n %= 1 << 64
    a, c = LCG_A, LCG_C
    acc_a, acc_c = 1, 0
    while n:
        if n & 1:
            acc_a, acc_c = (acc_a * a) & MASK64, (acc_c * a + c) & MASK64
        a, c = (a * a) & MASK64, (c * a + c) & MASK64
        n >>= 1
    return (state * acc_a + acc_c) & MASK64
