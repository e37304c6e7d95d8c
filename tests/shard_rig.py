"""What the tests of evaluation over a row-sharded entity table share (test_gpu_lp_shard, test_gpu_topk_shard,
test_gpu_relpred_shard): the one-process config, the rank worker's prologue and epilogue, the 2- and 4-rank runs on the
1003-entity typed graph, and the one-process config over the union of the ranks' tables.  Plain functions, no fixtures: each
test file keeps its own fixtures, port base and process-group timeout."""
import os
import sys

import numpy as np

from conftest import GOLDEN, ROOT

KG = os.path.join(GOLDEN, "kg_small")


def make_config(dim, path=KG, model="TransE", scale=3.0, relation=False):
    """One process over the whole table; `relation` sets the relation-prediction test flag instead of link prediction's."""
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(path)
    con.set_work_threads(1)
    con.set_dimension(dim)
    if relation:
        con.set_test_relation_prediction(True)
    else:
        con.set_test_link_prediction(True)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    if scale != 1.0:
        for t in con._tables:      # spread the scores: xavier-initialised tables rank almost at random
            t.mul_(scale)
        con.tables_changed()
    return con


def start_rank(rank, world, port, data, relation=False, **pg_args):
    """A rank worker's prologue: the gloo group (pg_args go to init_process_group), then a TransE D = 48 SGD config on `data`
    with its entity table sharded over the ranks, trained for four steps.  -> the Config."""
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, **pg_args)
    import openkeonspark_amd as pkg
    pkg._lib.lib().kge_set_option(b"inv_table_max_bytes", 0)
    con = pkg.Config()
    con.set_in_path(data)
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(48); con.set_nbatches(10)
    con.set_ent_neg_rate(3); con.set_alpha(0.02); con.set_opt_method("SGD")
    con.sparse_rows = True
    con.prefetch_sampling = False
    con.counts_min_records = 0
    if relation:
        con.set_test_relation_prediction(True)
    else:
        con.set_test_link_prediction(True)
    con.init()
    con.set_model_and_session(pkg.TransE)
    con.init_distributed()
    assert con._sharded("ent_embeddings") and con._tables[0].shape[0] == con._shard["chunk"]
    for _ in range(4):
        con.train_step()
    torch.cuda.synchronize()
    return con


def finish_rank(con, out_dir, world, rank, **results):
    """A rank worker's epilogue: `results` and the gathered tables (ent, rel) go to w<world>_r<rank>.npz."""
    import torch.distributed as dist
    params = con.get_parameters()      # (collective: the shards gathered; small tables only)
    np.savez(os.path.join(out_dir, "w%d_r%d.npz" % (world, rank)), ent=params["ent_embeddings"], rel=params["rel_embeddings"],
             **results)
    dist.barrier()
    dist.destroy_process_group()


def run_worlds(worker, base, port):
    """worker(rank, world, port, out_dir, data) on 2 and then 4 ranks over a 1003-entity typed graph written under `base`
    (a pathlib directory); 1003 divides by neither.  -> (out_dir, data)."""
    import torch.multiprocessing as mp
    from openkeonspark_amd import synthetic
    data = synthetic.make_typed_dataset(str(base / "kg1003"), synthetic.SMALL_TYPED, entities=1003, train=6000, valid=100, test=60)
    for i, w in enumerate((2, 4)):
        mp.start_processes(worker, args=(w, port + i, str(base), data), nprocs=w, join=True, start_method="spawn")
    return str(base), data


def load_ranks(out_dir, world):
    """What the `world` ranks' finish_rank wrote, by rank."""
    return [np.load(os.path.join(out_dir, "w%d_r%d.npz" % (world, g))) for g in range(world)]


def union_config(data, z, relation=False):
    """One process over the tables a rank gathered (every rank's are asserted equal by the tests)."""
    con = make_config(48, path=data, scale=1.0, relation=relation)
    con.set_parameters_by_name("ent_embeddings", z["ent"])
    con.set_parameters_by_name("rel_embeddings", z["rel"])
    return con
