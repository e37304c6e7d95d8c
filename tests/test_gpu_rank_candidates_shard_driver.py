"""Training driver on two ranks with the entity table sharded across them: early stop on validation MRR ranked against drawn
candidate lists (--early_stop_candidates) goes through the collective Config.validation_link_prediction_distributed(candidates=)
and logs what one process computes from the saved checkpoint."""
import datetime
import glob
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from shard_rig import KG, make_config

pytestmark = pytest.mark.gpu

PG_TIMEOUT = datetime.timedelta(seconds=60)
DIM, CANDIDATES, SEED = 32, 20, 3


def _driver_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    env = {"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world),
           "LOCAL_RANK": str(rank), "KGE_SINGLE_DEVICE": "1", "KGE_DIST_BACKEND": "gloo", "KGE_COUNTS_MIN_RECORDS": "0"}
    os.environ.update(env)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=PG_TIMEOUT)      # (the driver keeps a caller's group)
    from openkeonspark_amd import _lib
    from openkeonspark_amd import distribute_training as dt
    from openkeonspark_amd.Config import Config
    _lib.lib().kge_set_option(b"inv_table_max_bytes", 0)
    calls, plain = [], []
    real, real_plain = Config.validation_link_prediction_distributed, Config.validation_link_prediction

    def spy(self, **kw):
        counts, metrics = real(self, **kw)
        calls.append(dict(kw=kw, step=int(self.global_step), counts=counts.tolist(), metrics=metrics))
        return counts, metrics

    def spy_plain(self, *a, **kw):
        plain.append(1)
        return real_plain(self, *a, **kw)
    Config.validation_link_prediction_distributed = spy
    Config.validation_link_prediction = spy_plain
    # lr = 0: the tables stay what the checkpoint holds, the metric cannot improve and the run stops after `patience` checks
    args = ["--input_path", KG, "--output_path", os.path.join(out_dir, "run"), "--embedding_dimension", str(DIM),
            "--n_mini_batches", "3", "--ent_neg_rate", "3", "--alpha", "0.0", "--optimizer", "SGD", "--bern_flag", "1",
            "--train_times", "40", "--sparse_rows", "1", "--early_stop_patience", "2", "--debug", "1",
            "--early_stop_metric", "mrr", "--early_stop_candidates", str(CANDIDATES), "--early_stop_candidates_seed", str(SEED)]
    con = dt.main_fun(dt.parse_args(args))
    with open(os.path.join(out_dir, "calls_r%d.json" % rank), "w") as f:
        json.dump(dict(calls=calls, plain=len(plain), sharded=bool(con._sharded("ent_embeddings")), nbatches=int(con.nbatches),
                       step=int(con.global_step), valid=int(con.validTotal)), f)
    dist.barrier()
    dist.destroy_process_group()


def test_early_stop_on_mrr_against_drawn_candidates_on_a_sharded_table(tmp_path):
    import torch.multiprocessing as mp
    from openkeonspark_amd import distribute_training as dt
    from openkeonspark_amd.Config import Config
    assert "candidates" in Config.validation_link_prediction_distributed.__code__.co_varnames
    port = 41900 + os.getpid() % 1000
    mp.start_processes(_driver_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    logs = [json.load(open(str(tmp_path / ("calls_r%d.json" % g)))) for g in range(2)]
    for z in logs:
        assert z["sharded"] and z["plain"] == 0 and z["nbatches"] == 3
        # checks after epochs 1, 2 and 3: the first sets the best value, the next two run the patience out
        assert [c["step"] for c in z["calls"]] == [3, 6, 9] and z["step"] == 9
        assert all(c["kw"] == dict(test_head=False, sample=0, candidates=CANDIDATES, seed=SEED, type_constrained=False) for c in z["calls"])
    assert logs[0]["calls"] == logs[1]["calls"]           # the same counts and metric values on both ranks, check by check
    out = str(tmp_path / "run")
    assert os.path.exists(os.path.join(out, "stop.txt"))
    # one process over the checkpoint's tables
    main = sorted((p for p in glob.glob(os.path.join(out, "model.ckpt-*.npz")) if ".shard" not in p), key=lambda p: int(p[:-4].rsplit("-", 1)[1]))[-1]
    con = make_config(DIM, scale=1.0)
    ent, ent_total = dt.read_entity_rows(main[:-4], 0, con.entTotal, DIM)
    assert ent_total == con.entTotal
    con.set_parameters_by_name("ent_embeddings", ent)
    con.set_parameters_by_name("rel_embeddings", np.load(main)["rel_embeddings"])
    counts, metrics = con.validation_link_prediction(test_head=False, candidates=CANDIDATES, seed=SEED)
    assert counts.shape == (logs[0]["valid"], 2, 2) and counts[:, 0, 0].any() and not counts[:, 1].any()
    for c in logs[0]["calls"]:
        assert np.array_equal(np.asarray(c["counts"]), counts)
        assert c["metrics"] == metrics and 0.0 < c["metrics"]["r_filter_reci_rank"] <= 1.0
    # twenty candidates are not the whole table: the full ranking gives another value
    assert abs(metrics["r_filter_reci_rank"] - con.validation_link_prediction(test_head=False)[1]["r_filter_reci_rank"]) > 1e-6
