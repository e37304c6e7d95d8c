"""Training / evaluation driver: the loop of /root/reference/distribute_training.py without Spark or TF.

Same flags as `main_spark.py:299-324`, same `get_conf` (`distribute_training.py:32-71`), same per-step
log line (`:283`), same checkpoint discovery (`get_last_step`, `:134-156`: the step is parsed from the
`checkpoint` text file, `model.ckpt-<step>`), one checkpoint per epoch with `max_to_keep =
patience + 5` (`:103,226-234`), loss-based early stop with `stop.txt` (`:336-360`), new-entity growth
on restore (`main_spark.py:74-98`: xavier rows for parameters, zero rows for the Adam slots, rows of the initial value for Adagrad's accumulators).  One
process per GPU (torchrun) replaces the ps/worker cluster; rank 0 plays the chief.

A run whose entity table is sharded by row range (`--sparse_rows 1` on N ranks, SGD, LazyAdam, Adagrad or RowAdagrad) checkpoints without gathering
it: every rank writes its rows -- with LazyAdam their two moment rows, with Adagrad their accumulator rows, with RowAdagrad their one accumulator each too -- into `model.ckpt-<step>.shard<g>of<N>.npz` beside the
main file.  Such a checkpoint resumes at any number of ranks or in one process, a one-process checkpoint resumes sharded, and
new entities are grown on shards exactly as one process grows them.

    python -m openkeonspark_amd.distribute_training --input_path DATA/ --output_path OUT/ --model TransE ...
    torchrun --nproc-per-node 8 -m openkeonspark_amd.distribute_training ...

Early stop: both criteria of the reference -- validation accuracy of triple classification
(`:295-333`: thresholds from `getBestThreshold` on the validation positives / type-constrained
negatives of `getValidBatch`) when valid2id.txt / test2id.txt / type_constrain.txt are present, and the
loss (`:336-360`).  One deliberate difference: the reference then calls
`test_triple_classification(relThresh, valid_scores...)`, which walks the TEST set's per-relation
ranges over the validation score arrays (`Test.h:352-353` with `distribute_training.py:312`); here the
accuracy is computed over the validation triples the thresholds were fitted on.
"""
import argparse
import glob
import json
import os
import sys
import time
import zipfile

import numpy as np

from . import _lib
from .Config import Config, KgeError
from .Model import xavier_normal
from .TransD import TransD
from .TransE import TransE
from .TransH import TransH
from .TransR import TransR


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="OpenKEonSpark training loop on MI355X")
    p.add_argument("--cluster_size", type=int, default=1, help="accepted for compatibility (ranks come from torchrun)")
    p.add_argument("--num_ps", type=int, default=0, help="accepted for compatibility (no parameter servers)")
    p.add_argument("--num_gpus", type=int, default=1)
    p.add_argument("--cpp_lib_path", type=str, default=None)
    p.add_argument("--input_path", type=str, default=None)
    p.add_argument("--output_path", type=str, default=None)
    p.add_argument("--train_times", type=int, default=100)
    p.add_argument("--n_mini_batches", type=int, default=0)
    p.add_argument("--alpha", type=float, default=0.00001)
    p.add_argument("--margin", type=float, default=1.0)
    p.add_argument("--bern_flag", type=int, default=0)
    p.add_argument("--embedding_dimension", type=int, default=64)
    p.add_argument("--ent_dimension", type=int, default=0)
    p.add_argument("--rel_dimension", type=int, default=0)
    p.add_argument("--ent_neg_rate", type=int, default=1)
    p.add_argument("--rel_neg_rate", type=int, default=0)
    p.add_argument("--optimizer", type=str, default="SGD",
                   help="SGD (the default, and what any other name means), Adam (TF1's AdamOptimizer: every row moves every step), "
                        "LazyAdam (opt-in, non-parity: the Adam rule on the rows a step touches) or Adagrad (TF1's AdagradOptimizer, "
                        "accumulators from 0.1: on the touched rows for TransE / TransH / TransD, which is exactly the dense rule; one "
                        "accumulator table per parameter table, checkpointed as <var>/Adagrad; TransR in one process only) or RowAdagrad "
                        "(PyTorch-BigGraph's row-wise Adagrad: ONE accumulator per table row, which takes the row's mean squared "
                        "gradient, from 0.1 and without an epsilon; the same touched-rows paths, exact likewise; checkpointed as "
                        "<var>/RowAdagrad, float32 [rows]; TransR in one process only)")
    p.add_argument("--early_stop_patience", type=int, default=5)
    p.add_argument("--early_stop_stopping_step", type=int, default=1)
    p.add_argument("--early_stop_start_step", type=int, default=1)
    p.add_argument("--early_stop_metric", type=str, default="accuracy", choices=("accuracy", "hits10", "mrr"),
                   help="what an early-stop check measures on the validation split: accuracy = triple classification (the default), "
                        "hits10 / mrr = filtered Hits@10 / mean reciprocal rank of the validation triples (tail side; head side too with "
                        "--test_head 1), higher is better.  A ranking check scores every validation triple against every entity -- on a "
                        "large graph several training epochs of GPU time -- so rank against a drawn candidate list with "
                        "--early_stop_candidates (cost: triples x candidates instead of triples x entities), rank a sample of the "
                        "triples with --early_stop_rank_triples and / or check less often with --early_stop_stopping_step.  With an "
                        "entity table sharded across ranks "
                        "(--sparse_rows 1 on N ranks, TransE) the check is a collective: every rank ranks the triples against its own "
                        "rows and the counts are all-reduced, so every rank takes the same decision")
    p.add_argument("--early_stop_rank_triples", type=int, default=0,
                   help="hits10 / mrr: rank only this many validation triples, evenly spaced through valid2id.txt (0 = all of them)")
    p.add_argument("--early_stop_candidates", type=int, default=0,
                   help="hits10 / mrr: rank every chosen validation triple against this many candidates per side, drawn on the device "
                        "from a counter hash (Config.rank_triples_sampled; from the relation's type lists with "
                        "--type_constrained_sampling 1), instead of against every entity (0, the default).  With an entity table "
                        "sharded across ranks the check is the collective Config.validation_link_prediction_distributed(candidates=): "
                        "every rank ranks the candidates whose rows it owns and the counts are all-reduced")
    p.add_argument("--early_stop_candidates_seed", type=int, default=0,
                   help="seed of the drawn candidates; the same for every check of a run, so that successive checks are comparable")
    p.add_argument("--model", type=str, default="TransE")
    p.add_argument("--debug", type=int, default=0)
    p.add_argument("--mode", type=str, default="train")
    p.add_argument("--test_head", type=int, default=0)
    p.add_argument("--test_relation", type=int, default=0, help="1: --mode test also ranks the true relation of each test triple (rel* metrics)")
    p.add_argument("--test_roc", type=int, default=0, help="1: --mode test also gives the per-relation ROC AUC on the test split (roc_auc_macro, roc_auc_weighted)")
    p.add_argument("--work_threads", type=int, default=8, help="virtual sampler threads (Config.py:65 hard-codes 8)")
    p.add_argument("--seed", type=int, default=0, help="parameter initialisation seed")
    p.add_argument("--sparse_rows", type=int, default=-1, help="1 / 0: force / forbid the touched-rows-only update: TransE int8 records (SGD, or the opt-in non-parity "
                                                             "--optimizer LazyAdam; on N ranks the entity table is sharded by row range and each rank checkpoints its own rows "
                                                             "and moments), TransH / TransD float records "
                                                             "applied to the parameter rows in place (SGD, or --optimizer LazyAdam: the Adam rule on the rows a step "
                                                             "touches and on their moments; tables and moments replicated across ranks).  Default: automatic for "
                                                             "large tables; LazyAdam and Adagrad always take the touched-rows update (Adagrad's is exact: an element with zero "
                                                             "gradient keeps its value and its accumulator, so its checkpoints hold one accumulator row per parameter row)")
    p.add_argument("--shared_negatives_chunk", type=int, default=0,
                   help="P > 0: NON-PARITY, opt-in: chunks of P consecutive positives (1..127) share one set of --ent_neg_rate candidate "
                        "entities drawn from a hash of (--shared_negatives_seed, global step); pairs that are training triples are "
                        "masked (Config.set_shared_negatives).  TransE with SGD, LazyAdam or Adagrad; on N ranks the entity table is sharded "
                        "by row range (a width that is a multiple of 4) and the run equals the one-process run bit for bit; 0 = off "
                        "(default)")
    p.add_argument("--shared_negatives_seed", type=int, default=0, help="seed of the shared candidates' hash; a resumed run must repeat it")
    p.add_argument("--shared_negatives_by_relation", type=int, default=0,
                   help="1: with --shared_negatives_chunk P, the step's positives are ordered by relation and a chunk never crosses a "
                        "relation boundary (the run of a relation is cut into pieces of P); a candidate has one side for its chunk and, "
                        "with --type_constrained_sampling 1, comes from that side's type list of the chunk's relation "
                        "(Config.set_shared_negatives(..., by_relation=True)).  One rank only; a resumed run must repeat it.  "
                        "With --model TransH or TransD (widths up to 512) this is the one form of shared negatives: a chunk also "
                        "shares its relation's normal vector (TransD: transfer vector) and every candidate's projection.  With --model "
                        "TransR (rel_dim up to 512; SGD, Adagrad or Adam) likewise: a chunk shares its relation's matrix, and 2 P + N rows "
                        "go through the row GEMMs where the unshared step puts P (2 + N)")
    p.add_argument("--shared_negatives_in_chunk", type=int, default=0,
                   help="K > 0: with --shared_negatives_by_relation 1, K more candidates of every chunk are the chunk's own entities "
                        "(batch negatives: the tails, or heads, of its other positives, rotated by a hash of the step) beside the "
                        "--ent_neg_rate drawn ones; --ent_neg_rate + K <= 63 (Config.set_shared_negatives(..., in_chunk=K)).  "
                        "A resumed run must repeat it; 0 = off (default)")
    p.add_argument("--table_dtype", type=str, default="fp32", choices=("fp32", "bf16"),
                   help="bf16 (NON-PARITY, opt-in): TransE's tables are stored as bf16 -- half the memory and half the bytes of every "
                        "gather and touched-row update -- and trained on the one-rank int8-record touched-rows step with SGD or "
                        "RowAdagrad; updated rows are stored by stochastic rounding.  Checkpoints stay float32 (exact) and record the mode.  "
                        "With --shared_negatives_chunk P (one rank, widths up to 512, with or without --shared_negatives_by_relation) "
                        "the shared step gathers its 3 P + N rows per chunk from the bf16 tables; --table_rounding_seed and "
                        "--shared_negatives_seed must then differ (equal seeds, the defaults included, are refused: the two hashes would "
                        "share their bits)")
    p.add_argument("--table_rounding_seed", type=int, default=0,
                   help="seed of the stochastic rounding's hash (--table_dtype bf16); a resumed run must repeat it")
    p.add_argument("--bf16_evaluation", type=str, default="view", choices=("view", "stored"),
                   help="what the early stop on hits10 / mrr without --early_stop_candidates (and rank_triples, top-k entities) reads "
                        "with --table_dtype bf16: view = a cached float32 view of the tables (twice their bytes again, faster; the "
                        "stored rows where it cannot be allocated), stored = the stored bf16 rows themselves, the same metrics with "
                        "no memory of the table's size (Config.set_bf16_evaluation).  No effect on fp32 tables")
    p.add_argument("--type_constrained_sampling", type=int, default=0,
                   help="1: entity negatives of a training batch come from the relation's own head / tail type list "
                        "(type_constrain.txt in --input_path, required then) instead of from all entities; same random stream, "
                        "same positives (Config.set_type_constrained_sampling)")
    p.add_argument("--derive_type_constraints", type=int, default=0,
                   help="1: when type_constrain.txt is missing from --input_path, every rank derives the type lists from train + valid + "
                        "test (each relation's distinct heads and tails, as the reference's launcher regenerates them) and rank 0 also "
                        "writes the file; the accuracy early stop, --mode test's typed columns and --type_constrained_sampling 1 then "
                        "run as if the file had been there.  0 (the default): a missing file means none of those")
    return p.parse_args(argv)


def get_conf(argv):
    '''
    Set the Config class using the program args (distribute_training.py:32-71)
    '''
    con = Config(cpp_lib_path=argv.cpp_lib_path)
    con.set_in_path(argv.input_path)
    con.set_export_files(argv.output_path)
    if argv.mode != 'train':
        con.set_test_link_prediction(True)
    con.set_train_times(argv.train_times)
    con.set_nbatches(argv.n_mini_batches)
    con.set_alpha(argv.alpha)
    con.set_margin(argv.margin)
    con.set_bern(argv.bern_flag)
    if argv.ent_dimension != 0 and argv.rel_dimension != 0:
        con.set_ent_dimension(argv.ent_dimension)
        con.set_rel_dimension(argv.rel_dimension)
        con.hidden_size = argv.ent_dimension
    else:
        con.set_dimension(argv.embedding_dimension)
    con.set_ent_neg_rate(argv.ent_neg_rate)
    con.set_rel_neg_rate(argv.rel_neg_rate)
    con.set_opt_method(argv.optimizer)
    con.set_work_threads(getattr(argv, "work_threads", 8))
    con.seed = getattr(argv, "seed", 0)
    if getattr(argv, "sparse_rows", -1) >= 0:
        con.sparse_rows = bool(argv.sparse_rows)
    if getattr(argv, "shared_negatives_chunk", 0):
        con.set_shared_negatives(argv.shared_negatives_chunk, getattr(argv, "shared_negatives_seed", 0),
                                 by_relation=bool(getattr(argv, "shared_negatives_by_relation", 0)),
                                 in_chunk=getattr(argv, "shared_negatives_in_chunk", 0))
    if getattr(argv, "table_dtype", "fp32") != "fp32":
        con.set_table_dtype(argv.table_dtype, seed=getattr(argv, "table_rounding_seed", 0))
    con.set_bf16_evaluation(getattr(argv, "bf16_evaluation", "view"))
    typed = bool(getattr(argv, "type_constrained_sampling", 0))
    path = argv.input_path if not argv.input_path or argv.input_path.endswith("/") else argv.input_path + "/"
    derive = bool(getattr(argv, "derive_type_constraints", 0)) and bool(path) and not os.path.exists(path + "type_constrain.txt") and \
        all(os.path.exists(path + f) for f in ("valid2id.txt", "test2id.txt"))      # (the lists are derived from all three splits)
    con.set_type_constrained_sampling(typed and not derive)
    con.init()
    if derive:      # no type file: the lists from the triples, on every rank; the file from rank 0
        if not con.test_link_prediction:      # (init() imported the evaluation files otherwise)
            con.lib.kge_clear_error()
            con.lib.importTestFiles()
            _lib.raise_if_error(con.lib)
        con.derive_type_constraints(write=int(os.environ.get("RANK", "0")) == 0)
        if typed:
            con.set_type_constrained_sampling(True)
    name = argv.model.lower()
    con.set_model({"transh": TransH, "transr": TransR, "transd": TransD}.get(name, TransE))
    return con


# ---------------------------------------------------------------------------------------------
# checkpoints: TF Saver naming so that the reference's tooling finds the step
# ---------------------------------------------------------------------------------------------
def get_last_step(output_path):
    '''
    :return: last global step; 0 if there is no checkpoint (distribute_training.py:134-156)
    '''
    last_global_step = 0
    try:
        path = os.path.join(output_path, "checkpoint")
        if os.path.isfile(path):
            with open(path, "r") as f:
                line = f.readline().replace('"', '').split(":")[1].split("/")
                last_global_step = int(line[len(line) - 1].split("-")[1].strip())
    except Exception as e:  # same tolerance as the reference
        print("Error occured during last global step reading:")
        print(e)
    return last_global_step


def checkpoint_arrays(con):
    """Variables under the reference's names, Adam slots as `<var>/Adam`, `<var>/Adam_1`
    (main_spark.py:74-98), plus the optimiser scalars and the sampler's rng streams.  COLLECTIVE in data-parallel
    runs (owner-kept Adam slots are gathered): every rank calls it, rank 0 writes.  A SHARDED entity table (the
    table-sharded sparse mode) is not gathered: every rank writes its own rows -- and, with LazyAdam, their two moment rows --
    beside the main file (save_checkpoint); the main file holds what is replicated."""
    con.sync_optimizer_state()
    if con._sharded("ent_embeddings"):
        out = {n: t.detach().cpu().numpy() for n, t in con.trainModel.parameter_lists.items() if n != "ent_embeddings"}
    else:
        out = dict(con.get_parameters())
    if con._has_slots:
        for name, m, v in zip(con.trainModel.table_names, con._adam_m, con._adam_v):
            if con._sharded(name):
                continue      # shard-sized: in this rank's shard file as `adam` / `adam_1`
            out[name + "/Adam"] = m.detach().cpu().numpy()
            out[name + "/Adam_1"] = v.detach().cpu().numpy()
        out["beta1_power"] = np.float32(con._beta1_power)
        out["beta2_power"] = np.float32(con._beta2_power)
    if getattr(con, "_adagrad", False):      # TF's slot name; a shard-sized accumulator is in this rank's shard file as `adagrad`
        for name, a in zip(con.trainModel.table_names, con._adagrad_acc):
            if not con._sharded(name):
                out[name + "/Adagrad"] = a.detach().cpu().numpy()
    if getattr(con, "_row_adagrad", False):  # one float per row, float32 [rows]; a shard-sized one is in the shard file as `rowadagrad`
        for name, a in zip(con.trainModel.table_names, con._rowadagrad_acc):
            if not con._sharded(name):
                out[name + "/RowAdagrad"] = a.detach().cpu().numpy()
    out["global_step"] = np.int64(con.global_step)
    if getattr(con, "_bf16", False):      # bf16 table storage: the arrays above are float32 (an exact widening); the mode and its rounding seed
        out["table_dtype"] = table_dtype_record(con)
    if getattr(con, "_shared_chunk", 0):      # shared negatives: the candidates are a hash of (seed, global_step), chunked by `chunk`
        out["shared_negatives"] = shared_negatives_record(con)
    # with sampling one step ahead the device streams are one batch further than the training: store the states the
    # NEXT step's batch starts from, so that a resumed run trains on exactly the batches an uninterrupted one would
    out["rng_streams"] = con.get_stream_states(before_prefetch=True)
    return out


def table_dtype_record(con):
    """What a checkpoint keeps of a run's bf16 table storage: uint64 [1, rounding seed].  An fp32 run writes no record."""
    return np.array([1, int(getattr(con, "_table_seed", 0))], dtype=np.uint64)


def check_table_dtype_record(z, con):
    """bf16 table storage across a resume.  The stored arrays are float32 either way, so an fp32 run resumes from a bf16
    checkpoint as from any other, and a bf16 run from an fp32 one -- its tables are rounded to nearest-even once, which is said.
    A bf16 run that resumes a bf16 checkpoint must repeat the rounding seed: the resumed run then equals the uninterrupted one
    bit for bit (the hash depends on the seed and the global step only)."""
    if not getattr(con, "_bf16", False):
        return
    if "table_dtype" not in z:
        print("restore: the checkpoint holds fp32 tables; this run stores bf16 tables: they are rounded to nearest-even once")
        return
    was = [int(x) for x in np.asarray(z["table_dtype"]).reshape(-1)]
    if was[0] == 1 and was[1] != int(con._table_seed):
        raise KgeError("the checkpoint was written with bf16 table storage and rounding seed %d, this run has %d: resume with the "
                       "same --table_rounding_seed" % (was[1], int(con._table_seed)))


def _shared_negatives_mode(con):
    """(chunk, seed, by_relation, typed) of a Config's shared negatives; all zero when they are off.  typed: the candidates come
    from the relations' type lists (type-constrained sampling on relation-grouped chunks)."""
    chunk = int(getattr(con, "_shared_chunk", 0))
    if not chunk:
        return (0, 0, 0, 0)
    by_relation = int(bool(getattr(con, "_shared_by_relation", False)))
    return (chunk, int(getattr(con, "_shared_seed", 0)), by_relation, int(bool(by_relation and con.type_constrained_sampling)))


def _shared_in_chunk(con):
    """K of a Config's in-chunk candidates (Config.set_shared_negatives(..., in_chunk=K)); 0 when they, or shared negatives, are off."""
    return int(getattr(con, "_shared_in_chunk", 0)) if int(getattr(con, "_shared_chunk", 0)) else 0


def shared_negatives_record(con):
    """What a checkpoint keeps of a run's shared negatives: uint64 [chunk, seed], and [chunk, seed, by_relation, typed] when the
    chunks are relation-grouped (a record of two means False for both); a fifth field, in_chunk, only when it is not 0, so every
    record without in-chunk candidates keeps its length."""
    mode = _shared_negatives_mode(con)
    k = _shared_in_chunk(con)
    return np.array(mode + (k,) if k else mode if mode[2] or mode[3] else mode[:2], dtype=np.uint64)


def check_shared_negatives_record(z, con):
    """A resumed run must draw the candidates the interrupted one would have drawn: refuse a checkpoint (its arrays `z`) whose
    shared-negatives record differs from this run's."""
    was = tuple(int(x) for x in z["shared_negatives"]) if "shared_negatives" in z else (0, 0)
    was = (was + (0, 0, 0))[:5]      # (a checkpoint without by_relation / typed / in_chunk: all off)
    was, was_k = was[:4], was[4]
    now, now_k = _shared_negatives_mode(con), _shared_in_chunk(con)
    if was != now and not (was[2] or was[3] or now[2] or now[3]):      # chunks by position on both sides: the two fields alone
        raise KgeError("the checkpoint was written with shared negatives (chunk, seed) = %s, this run has %s: resume with the same "
                       "--shared_negatives_chunk / --shared_negatives_seed (0 0 = off)" % (was[:2], now[:2]))
    if was != now:
        raise KgeError("the checkpoint was written with shared negatives (chunk, seed, by_relation, typed) = %s, this run has %s: resume "
                       "with the same --shared_negatives_chunk / --shared_negatives_seed / --shared_negatives_by_relation / "
                       "--type_constrained_sampling (all 0 = off)" % (was, now))
    if was_k != now_k:
        raise KgeError("the checkpoint was written with %d in-chunk candidates per chunk of shared negatives, this run has %d: resume "
                       "with the same --shared_negatives_in_chunk (0 = off)" % (was_k, now_k))


def _step_of(path):
    return int(os.path.basename(path).split("model.ckpt-")[1].split(".")[0])


def _atomic_savez(path, **arrays):
    """np.savez under a temporary name, renamed into place: a reader (or a crash) never sees a half-written file.  A value may
    be a callable returning the array: it is called when its member is written and dropped right after, so that a shard file
    of several shard-sized arrays holds one of them in host memory at a time (np.savez's own layout: stored, zip64)."""
    tmp = path + ".tmp%d" % os.getpid()
    with zipfile.ZipFile(tmp, mode="w", compression=zipfile.ZIP_STORED, allowZip64=True) as zf:
        for key, val in arrays.items():
            with zf.open(key + ".npy", "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(val() if callable(val) else val), allow_pickle=False)
    os.replace(tmp, path)


def save_checkpoint(con, output_path, max_to_keep=10, write=True):
    """COLLECTIVE in data-parallel runs.  Order of a SHARDED checkpoint (needs an `output_path` every rank can write and, on
    restore, read -- a shared directory): every rank writes its shard file -> barrier -> rank 0 writes the main file and only
    THEN the `checkpoint` pointer, then prunes.  The pointer therefore never names a step whose shard files are incomplete, and
    older complete checkpoints are deleted only after the new one is whole.  A shard file holds `rows` (this rank's rows
    [lo, hi) of the entity table), `lo`, `hi`, `ent_total` and, for LazyAdam, the moment rows `adam` / `adam_1` of the same range."""
    arrays = checkpoint_arrays(con)
    step = con.global_step
    base = os.path.join(output_path, "model.ckpt-%d" % step)
    if con._sharded("ent_embeddings"):      # this rank's rows of the entity table: model.ckpt-<step>.shard<g>of<N>.npz
        os.makedirs(output_path, exist_ok=True)
        sh = con._shard
        n = sh["hi"] - sh["lo"]
        host = lambda t: (lambda: t[:n].detach().cpu().numpy())
        parts = dict(rows=host(con.trainModel.parameter_lists["ent_embeddings"]), lo=np.int64(sh["lo"]), hi=np.int64(sh["hi"]),
                     ent_total=np.int64(con.entTotal))
        if con._has_slots:     # LazyAdam: the moment rows travel with their entity rows
            parts.update(adam=host(con._adam_m[0]), adam_1=host(con._adam_v[0]))
        if getattr(con, "_adagrad", False):     # Adagrad: the accumulator rows do
            parts.update(adagrad=host(con._adagrad_acc[0]))
        if getattr(con, "_row_adagrad", False): # RowAdagrad: one accumulator per entity row
            parts.update(rowadagrad=host(con._rowadagrad_acc[0]))
        _atomic_savez(base + ".shard%dof%d.npz" % (con.rank, con.world_size), **parts)
        import torch.distributed as dist
        con.comm_fence("pg")
        dist.barrier(group=getattr(con, "_pg", None))      # all shard files of this step exist before anything points at them
    if not write:
        return None
    os.makedirs(output_path, exist_ok=True)
    _atomic_savez(base + ".npz", **{k.replace("/", "__"): v for k, v in arrays.items()})
    tmp = os.path.join(output_path, "checkpoint.tmp%d" % os.getpid())
    with open(tmp, "w") as f:
        f.write('model_checkpoint_path: "%s"\n' % base)
    os.replace(tmp, os.path.join(output_path, "checkpoint"))
    kept = sorted((p for p in glob.glob(os.path.join(output_path, "model.ckpt-*.npz")) if ".shard" not in p), key=_step_of)
    for old in kept[:-max_to_keep]:
        for part in glob.glob(old[:-4] + ".shard*of*.npz"):
            os.remove(part)
        os.remove(old)
    return base + ".npz"


def shard_files(base, keys=("rows",)):
    """The shard files of the sharded checkpoint `base` (model.ckpt-<step>) as [(path, lo, hi)] sorted by `lo`, and the entity
    count they were written for.  Checked before anything is read -- every rank sees the same files and so fails the same way,
    none is left waiting in a collective: the files must tile [0, ent_total) and each must hold the arrays `keys`."""
    parts, totals = [], set()
    for path in glob.glob(base + ".shard*of*.npz"):
        with np.load(path) as z:
            missing = [k for k in keys if k not in z.files]
            if missing:
                raise ValueError("sharded checkpoint %s: shard file %s has no %s" % (base, os.path.basename(path), ", ".join(missing)))
            parts.append((path, int(z["lo"]), int(z["hi"])))
            totals.add(int(z["ent_total"]))
    if len(totals) != 1:
        raise ValueError("sharded checkpoint %s: %s" % (base, "no shard files" if not totals else
                                                        "shard files of different entity counts %s" % sorted(totals)))
    ent_total = totals.pop()
    parts.sort(key=lambda p: p[1])
    end = 0
    for _, lo, hi in parts:
        if lo > end:
            break
        end = max(end, hi)
    if end < ent_total:
        raise ValueError("sharded checkpoint %s: entity rows [%d, %d) are not in any of its shard files" % (base, end, ent_total))
    return parts, ent_total


def read_entity_rows(base, lo, hi, dim, key="rows", parts=None, fill=0.0):
    """Rows [lo, hi) of the array `key` of a sharded checkpoint -- `rows`: the entity table, `adam` / `adam_1`: its LazyAdam
    moments, `adagrad`: its Adagrad accumulators -- from whichever shard files hold them (the number of ranks may differ from the run that wrote them).  Returns
    (array of hi - lo rows, ent_total): rows at or beyond the checkpoint's entity count `ent_total` are NEW entities, left at
    `fill` (zero: for the caller to fill, or an Adam moment; an Adagrad accumulator starts at its initial value); a row below it that no shard file holds is an error (shard_files; `parts`: its result)."""
    parts, ent_total = parts if parts is not None else shard_files(base, (key,))
    out = np.full((hi - lo,) if dim is None else (hi - lo, dim), fill, np.float32)     # dim None: one value per row (`rowadagrad`)
    for path, plo, phi in parts:
        a, b = max(lo, plo), min(hi, phi, ent_total)
        if a < b:
            with np.load(path) as z:
                out[a - lo:b - lo] = z[key][a - plo:b - plo]
    return out, ent_total


def slot_keys(z, adam_slots, adagrad, row_adagrad=False):
    """Which arrays a shard file must hold beside `rows` for a run with these optimizer slots resuming the checkpoint whose main
    file is `z`: the two moment arrays where an Adam-family run resumes an Adam-family checkpoint (it has `beta1_power`), the
    accumulator where an Adagrad run resumes an Adagrad checkpoint (its replicated tables have `<var>/Adagrad`), the per-row
    accumulator `rowadagrad` where a RowAdagrad run resumes a RowAdagrad checkpoint (`<var>/RowAdagrad`).  Anything else
    -- an SGD checkpoint, or slots the new run has no use for -- reads the rows alone: the run starts from fresh slots."""
    keys = ("rows",)
    if adam_slots and "beta1_power" in z:
        keys += ("adam", "adam_1")
    if adagrad and any(k.endswith("/Adagrad") for k in z):
        keys += ("adagrad",)
    if row_adagrad and any(k.endswith("/RowAdagrad") for k in z):
        keys += ("rowadagrad",)
    return keys


def grow_table(table, rows, rng, zeros=False, fill=0.0):
    """Append rows for new entities (main_spark.py:74-98): xavier-initialised for a parameter table,
    zeros for an Adam slot, `fill` (with zeros=True) for an Adagrad accumulator, whose rows start at its initial value.  The reference draws the WHOLE [final rows, dim] variable with the xavier
    initializer (main_spark.py:78) and keeps its tail, so the new rows' stddev is sqrt(2.6/(rows+dim))
    with rows = the final row count, not the number of appended rows."""
    table = np.asarray(table, dtype=np.float32)
    extra = rows - table.shape[0]
    if extra <= 0:
        return table
    new = (np.full((extra, table.shape[1]), fill, np.float32) if zeros
           else xavier_normal(rng, (extra, table.shape[1]), fan_in=rows))
    return np.concatenate([table, new], axis=0)


def _set_slots(con, i, name, m, v):
    """Adam moments of table i from whole-table arrays; a sharded entity table keeps its rows [lo, hi)."""
    import torch
    for slots, full in ((con._adam_m, m), (con._adam_v, v)):
        if con._sharded(name):
            lo, hi = con._shard["lo"], con._shard["hi"]
            slots[i][:hi - lo].copy_(torch.from_numpy(np.ascontiguousarray(full[lo:hi])))
        else:
            slots[i].copy_(torch.from_numpy(full))


def _set_accumulator(con, i, name, acc):
    """Adagrad accumulator of table i from a whole-table array; a sharded entity table keeps its rows [lo, hi)."""
    import torch
    if con._sharded(name):
        lo, hi = con._shard["lo"], con._shard["hi"]
        con._adagrad_acc[i][:hi - lo].copy_(torch.from_numpy(np.ascontiguousarray(acc[lo:hi])))
    else:
        con._adagrad_acc[i].copy_(torch.from_numpy(np.ascontiguousarray(acc.reshape(tuple(con._adagrad_acc[i].shape)))))


def _set_row_accumulator(con, i, name, acc):
    """RowAdagrad accumulator of table i from a whole [rows] array; a sharded entity table keeps its rows [lo, hi)."""
    import torch
    if con._sharded(name):
        lo, hi = con._shard["lo"], con._shard["hi"]
        con._rowadagrad_acc[i][:hi - lo].copy_(torch.from_numpy(np.ascontiguousarray(acc[lo:hi])))
    else:
        con._rowadagrad_acc[i].copy_(torch.from_numpy(np.ascontiguousarray(acc)))


def _restore_sharded_rows(con, i, name, base, z, rows, dim, allow_growth, rng):
    """Table i (the entity table) from the shard files of a sharded checkpoint, into this rank's shard [lo, hi) of the new run or,
    in one process, whole.  Rows of entities the checkpoint does not know are grown as one process grows them (grow_table):
    every rank draws the same xavier block for rows [ent_total, rows) from `rng` and keeps its own part; their moments are zero.
    An Adam-family checkpoint (it has `beta1_power`) resumed with slots must carry the moment rows in its shard files; an SGD
    checkpoint resumed with slots starts from zero moments.  Adagrad alike (slot_keys): its accumulator rows come from the shard
    files' `adagrad`, new entities' rows -- and every row, from a checkpoint without accumulators -- hold the initial value.
    RowAdagrad the same with `rowadagrad`, one value per row."""
    import torch
    adagrad, row_adagrad = getattr(con, "_adagrad", False), getattr(con, "_row_adagrad", False)
    keys = slot_keys(z, con._has_slots, adagrad, row_adagrad)
    parts = shard_files(base, keys)
    ent_total = parts[1]
    if rows != ent_total and (not allow_growth or rows < ent_total):
        raise ValueError("checkpoint table %s has %d rows, model needs %d" % (name, ent_total, rows))
    new = xavier_normal(rng, (rows - ent_total, dim), fan_in=rows) if rows > ent_total else None
    lo, hi = (con._shard["lo"], con._shard["hi"]) if con._sharded(name) else (0, rows)
    if hi <= lo:
        return
    dsts = dict(rows=con._tables[i])
    if "adam" in keys:
        dsts.update(adam=con._adam_m[i], adam_1=con._adam_v[i])
    if "adagrad" in keys:
        dsts.update(adagrad=con._adagrad_acc[i])
    elif adagrad:
        con._adagrad_acc[i].fill_(float(con.adagrad_initial_accumulator))
    if "rowadagrad" in keys:
        dsts.update(rowadagrad=con._rowadagrad_acc[i])
    elif row_adagrad:
        con._rowadagrad_acc[i].fill_(float(con.adagrad_initial_accumulator))
    for key, dst in dsts.items():
        part, _ = read_entity_rows(base, lo, hi, None if key == "rowadagrad" else dim, key, parts,
                                   fill=float(con.adagrad_initial_accumulator) if key in ("adagrad", "rowadagrad") else 0.0)
        if key == "rows" and new is not None and hi > ent_total:
            a = max(lo, ent_total)
            part[a - lo:] = new[a - ent_total:hi - ent_total]
        dst[:hi - lo].copy_(torch.from_numpy(part))
        del part
    con.tables_changed()


def restore_checkpoint(con, path, allow_growth=True, arrays=None):
    """Load a checkpoint into an initialised Config (after set_model_and_session).  If the dataset
    gained entities since the checkpoint was written, entity tables are grown as the reference's
    `update_entities_and_model` does.  `arrays`: the checkpoint's contents when they were read elsewhere
    (rank 0 reads the file and broadcasts it: for replicated tables the other ranks need not see the output directory; a
    SHARDED entity table is read by every rank from the shard files, so that mode needs a shared `output_path`).  Sharded and
    whole checkpoints restore into sharded and one-process runs alike, at any number of ranks: a rank takes its rows [lo, hi)
    of the entity table (and of its LazyAdam moments) from whichever file holds them."""
    z = arrays if arrays is not None else {k.replace("__", "/"): v for k, v in np.load(path).items()}
    # shared negatives: a resumed run must draw the candidates the interrupted one would have drawn
    check_shared_negatives_record(z, con)
    check_table_dtype_record(z, con)
    rng = np.random.default_rng(getattr(con, "seed", 0) + 1)
    shapes = con.trainModel.table_shapes()
    for i, name in enumerate(con.trainModel.table_names):
        rows = shapes[name][0]
        if name not in z:      # a sharded checkpoint: the entity rows live in per-rank shard files beside the main file
            base = path[:-4] if path.endswith(".npz") else path
            _restore_sharded_rows(con, i, name, base, z, rows, shapes[name][1], allow_growth, rng)
            continue
        tab = z[name]
        if tab.shape[0] != rows:
            if not allow_growth or tab.shape[0] > rows:
                raise ValueError("checkpoint table %s has %d rows, model needs %d" % (name, tab.shape[0], rows))
            tab = grow_table(tab, rows, rng)
        con.set_parameters_by_name(name, tab)
        if con._has_slots and name + "/Adam" in z:
            _set_slots(con, i, name, grow_table(z[name + "/Adam"], rows, rng, zeros=True),
                       grow_table(z[name + "/Adam_1"], rows, rng, zeros=True))
        if getattr(con, "_adagrad", False):      # absent (an SGD checkpoint, say): fresh accumulators
            a0 = float(con.adagrad_initial_accumulator)
            acc = grow_table(z[name + "/Adagrad"], rows, rng, zeros=True, fill=a0) if name + "/Adagrad" in z else \
                np.full((rows, shapes[name][1]), a0, np.float32)
            _set_accumulator(con, i, name, acc)
        if getattr(con, "_row_adagrad", False):  # likewise; rows of new entities start at the initial value
            acc = np.full(rows, float(con.adagrad_initial_accumulator), np.float32)
            if name + "/RowAdagrad" in z:
                old = np.asarray(z[name + "/RowAdagrad"], np.float32).reshape(-1)
                if old.shape[0] > rows:
                    raise ValueError("checkpoint accumulator %s/RowAdagrad has %d rows, model needs %d" % (name, old.shape[0], rows))
                acc[:old.shape[0]] = old
            _set_row_accumulator(con, i, name, acc)
    if con._has_slots and "beta1_power" in z:
        con._beta1_power = np.float32(z["beta1_power"])
        con._beta2_power = np.float32(z["beta2_power"])
    con.global_step = int(z.get("global_step", 0))
    if "rng_streams" in z and len(z["rng_streams"]) == con.workThreads:
        import torch
        s = np.ascontiguousarray(z["rng_streams"], dtype=np.uint64)
        if torch.cuda.is_available():
            torch.cuda.synchronize()   # a sampler prefetched on the side stream may still be writing the other half of the state buffer
        con.lib.kge_set_stream_states(s.ctypes.data, con.workThreads)
        con._prefetched = None     # a batch drawn ahead belongs to the run that was interrupted
    return con.global_step


# ---------------------------------------------------------------------------------------------
def _init_validation(con, argv):
    """getValidBatch once before the loop (distribute_training.py:262): validation positives and their
    type-constrained negatives, or None when the evaluation files are absent."""
    path = con.in_path if con.in_path.endswith("/") else con.in_path + "/"
    derived = getattr(con, "_type_lists_from", None) == "derived"      # --derive_type_constraints 1: the lists need no file
    if not all(os.path.exists(path + f) for f in ("valid2id.txt", "test2id.txt") + (() if derived else ("type_constrain.txt",))):
        return None
    import ctypes
    L = con.lib
    L.kge_clear_error()
    L.importTestFiles()
    if derived:
        con.derive_type_constraints()
    else:
        L.importTypeFiles()
    _lib.raise_if_error(L)
    n = L.getValidTotal()
    arrs = [np.zeros(n, np.int64) for _ in range(6)]
    L.getValidBatch.argtypes = [ctypes.c_void_p] * 6
    L.getBestThreshold.argtypes = [ctypes.c_void_p] * 3
    L.getValidBatch(*[a.ctypes.data for a in arrs])
    _lib.raise_if_error(L)
    return arrs


def _validation_accuracy(con, valid):
    """Thresholds fitted on the validation scores, then the share of the 2 V answers they get right: on the device
    (Config.validation_accuracy: ids uploaded once, four counts read back), on the host where the entity table is sharded."""
    return con.validation_accuracy(valid)


def _init_rank_validation(con):
    """The files a ranking early-stop check needs (Config.init_link_prediction); None when valid2id.txt / test2id.txt are absent."""
    path = con.in_path if con.in_path.endswith("/") else con.in_path + "/"
    if not all(os.path.exists(path + f) for f in ("valid2id.txt", "test2id.txt")):
        return None
    con.init_link_prediction()
    return True


def _validation_rank_metric(con, argv):
    """Filtered Hits@10 or MRR of the validation triples, the mean over the ranked sides (Config.validation_link_prediction).
    With replicated tables every rank ranks the same triples itself: identical tables, identical decisions, no collective.
    With a sharded entity table it is the collective Config.validation_link_prediction_distributed: every rank reaches the
    check at the same global step and receives the same all-reduced counts, so the decisions agree without a broadcast."""
    test_head = bool(argv.test_head)
    name = "_filter_tot" if argv.early_stop_metric == "hits10" else "_filter_reci_rank"
    sides = ("r", "l") if test_head else ("r",)
    if argv.early_stop_candidates > 0:      # drawn candidate lists; on a sharded entity table every rank counts the candidates it owns
        rank_valid = con.validation_link_prediction_distributed if con._sharded("ent_embeddings") else con.validation_link_prediction
        metrics = rank_valid(test_head=test_head, sample=argv.early_stop_rank_triples, candidates=argv.early_stop_candidates,
                             seed=argv.early_stop_candidates_seed, type_constrained=bool(argv.type_constrained_sampling))[1]
        return sum(metrics[p + name] for p in sides) / len(sides)
    rank_valid = con.validation_link_prediction_distributed if con._sharded("ent_embeddings") else con.validation_link_prediction
    metrics = rank_valid(test_head=test_head, sample=argv.early_stop_rank_triples)[1]
    return sum(metrics[p + name] for p in sides) / len(sides)


def main_fun(argv):
    """Train or evaluate (distribute_training.py:161-612)."""
    import torch
    distributed = int(os.environ.get("WORLD_SIZE", "1")) > 1
    rank = int(os.environ.get("RANK", "0"))
    if distributed:
        import torch.distributed as dist
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if os.environ.get("KGE_SINGLE_DEVICE") == "1":
            local_rank = 0        # rehearsal of the multi-rank path on a one-GPU box (with KGE_DIST_BACKEND=gloo)
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        own_group = not dist.is_initialized()       # a caller that brought its own process group keeps it afterwards
        if own_group:
            dist.init_process_group(os.environ.get("KGE_DIST_BACKEND", "nccl"))   # "nccl" is RCCL on ROCm
    con = get_conf(argv)
    con.device = "cuda:%d" % torch.cuda.current_device()
    con.set_model_and_session(con.model)
    if distributed:
        con.init_distributed()
    last_global_step = get_last_step(argv.output_path) if (argv.output_path and rank == 0) else 0
    arrays = None
    if distributed:   # rank 0 decides: the other ranks need not see the output directory
        box = [last_global_step, None]
        if rank == 0 and last_global_step > 0:
            path = os.path.join(argv.output_path, "model.ckpt-%d.npz" % last_global_step)
            box[1] = {k.replace("__", "/"): v for k, v in np.load(path).items()}
        dist.broadcast_object_list(box, src=0)
        last_global_step, arrays = box
    if last_global_step > 0:
        restore_checkpoint(con, os.path.join(argv.output_path, "model.ckpt-%d.npz" % last_global_step), arrays=arrays)

    if argv.mode != "train":
        if argv.test_roc and con._sharded("ent_embeddings"):      # before the rankers run, not after them
            raise KgeError("--test_roc over an entity table sharded across ranks is not supported (Config.roc_auc refuses it)")
        if distributed:   # one contiguous slice of the test set per rank, accumulators all-reduced
            metrics = con.link_prediction_distributed(test_head=bool(argv.test_head))
            if argv.test_relation:
                metrics.update(con.relation_prediction_distributed())
        else:
            out, metrics = con.link_prediction(test_head=bool(argv.test_head))
            if argv.test_relation:
                metrics.update(con.relation_prediction()[1])
        if argv.test_roc:      # every rank draws and scores the same lists
            roc = con.roc_auc("test")
            # None (JSON null) when no relation has both validation and test triples: a bare NaN is not JSON
            metrics.update({"roc_auc_" + k: (None if roc[k] != roc[k] else roc[k]) for k in ("macro", "weighted")})
        if rank == 0:
            print(json.dumps(metrics, indent=1))
            if argv.output_path:
                with open(os.path.join(argv.output_path, "lp_results.json"), "w") as f:
                    json.dump(metrics, f, indent=1)
        return metrics

    metric = argv.early_stop_metric
    if argv.early_stop_candidates < 0:
        raise KgeError("--early_stop_candidates must be >= 0, got %d" % argv.early_stop_candidates)
    valid = _init_validation(con, argv) if metric == "accuracy" else _init_rank_validation(con)
    best_acc, wait_steps_acc, best_step_acc = -1.0, 0, last_global_step
    iterations = con.train_times * con.nbatches + last_global_step      # distribute_training.py:205
    patience = argv.early_stop_patience
    stopping_step = argv.early_stop_stopping_step * con.nbatches
    to_reach_step = argv.early_stop_start_step * con.nbatches + last_global_step
    best_loss, wait_steps_loss, best_step = float("inf"), 0, last_global_step
    t0 = time.time()
    g = last_global_step
    while g < iterations:
        if not distributed and con.persistent_preferred():
            # launch-latency-bound step sizes: every step up to the next checkpoint / early-stop check in ONE persistent launch
            # (csrc/persist.hip); the per-step log lines of distribute_training.py:283 are printed from the returned losses
            to_epoch = con.nbatches - (g - last_global_step) % con.nbatches
            chunk = min(iterations - g, to_epoch, max(to_reach_step - g, 1) if g < to_reach_step else to_epoch)
            losses = con.train_steps(chunk)
            for i, l in enumerate(losses):
                gi = g + i + 1
                print('Global step: {} Epoch: {} Batch: {} loss: {}'.format(
                    gi, int((gi - last_global_step) / con.nbatches), int((gi - last_global_step) % con.nbatches), float(l)))
            loss = float(losses[-1])
            g = con.global_step
        else:
            loss = con.train_step()
            g = con.global_step
            if rank == 0:
                print('Global step: {} Epoch: {} Batch: {} loss: {}'.format(
                    g, int((g - last_global_step) / con.nbatches), int((g - last_global_step) % con.nbatches), loss))
        if (g - last_global_step) % con.nbatches == 0 and argv.output_path:
            save_checkpoint(con, argv.output_path, max_to_keep=patience + 5, write=rank == 0)
        if g < iterations and g >= to_reach_step:
            while g >= to_reach_step:
                to_reach_step += stopping_step
            if valid is not None:   # accuracy criterion of distribute_training.py:295-333, or validation Hits@10 / MRR in its place
                acc = _validation_accuracy(con, valid) if metric == "accuracy" else _validation_rank_metric(con, argv)
                if argv.debug and rank == 0:
                    print("[ Early Stop Check (%s) ] best %.10f now %.10f" % ("Accuracy" if metric == "accuracy" else metric, best_acc, acc))
                if acc > best_acc:
                    best_acc, wait_steps_acc, best_step_acc = acc, 0, g
                elif wait_steps_acc < patience:
                    wait_steps_acc += 1
                if wait_steps_acc >= patience:
                    if rank == 0:
                        what = "Accuracy" if metric == "accuracy" else metric
                        print('{} early stop. {} has not been improved enough in {} times'.format(what, what, patience))
                        if argv.output_path:
                            with open(os.path.join(argv.output_path, "stop.txt"), "w") as f:
                                f.write(str(best_step_acc) + "\n")
                    break
            # loss criterion of distribute_training.py:336-360 (every rank sees the same all-reduced loss)
            if loss < best_loss:
                best_loss, wait_steps_loss, best_step = loss, 0, g
            elif wait_steps_loss < patience:
                wait_steps_loss += 1
            if wait_steps_loss >= patience:
                if rank == 0:
                    print('Loss early stop. Losses has not been improved enough in {} times'.format(patience))
                    if argv.output_path:
                        with open(os.path.join(argv.output_path, "stop.txt"), "w") as f:
                            f.write(str(best_step) + "\n")
                break
    if argv.output_path:
        save_checkpoint(con, argv.output_path, max_to_keep=patience + 5, write=rank == 0)
        if rank == 0:
            with open(os.path.join(argv.output_path, "time.txt"), "w") as f:   # main_spark.py:339-344
                f.write(str(time.time() - t0))
    if distributed:
        import torch.distributed as dist
        con.comm_fence("pg")
        dist.barrier()
        if own_group:
            dist.destroy_process_group()
    return con


if __name__ == "__main__":
    main_fun(parse_args())
