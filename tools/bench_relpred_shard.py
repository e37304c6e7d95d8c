#!/usr/bin/env python3
"""Relation prediction with the entity rows supplied by the caller (kge_relation_prediction_rows, the ranker of a table sharded
across ranks): one JSON line per workload, a host clock around synchronised calls after a warm-up, counts checked against
kge_relation_prediction on the same table.
  (a) the FB15k-237-shaped test set (synthetic.FB15K237_TYPED: 14 541 entities, 237 relations, 20 466 test triples, TransE
      D = 200): kge_relation_prediction_rows with the query rows already gathered, against kge_relation_prediction;
  (b) the same graph through the whole sharded Config.relation_prediction on one GPU: a one-rank RCCL group with
      Config.force_data_parallel, which shards the table into one shard.  The row exchange (kge_test_entity_ids,
      shard_eval.query_rows, as relation_prediction runs them) is timed on its own and reported as a share of the call.
Kernel times: run under `rocprofv3 --kernel-trace --stats` (relpred_score_kernel, relpred_rank_kernel, relpred_iota_kernel).
usage: bench_relpred_shard.py [--which a,b] [--reps R] [--dir DIR]"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

DIM = 200


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def make_config(d, sharded):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(d); con.set_work_threads(8); con.set_dimension(DIM)
    con.set_test_relation_prediction(True)
    if sharded:
        con.sparse_rows = True
    con.init()
    con.set_model_and_session(pkg.TransE)
    for t in con._tables:
        t.mul_(3.0)
    con.tables_changed()
    if sharded:
        con.force_data_parallel = True
        con.init_distributed()
        assert con._sharded("ent_embeddings") and con._shard["hi"] - con._shard["lo"] == con.entTotal
    return con


def reference_counts(con, count):
    from openkeonspark_amd import _lib
    out = np.zeros((count, 4), dtype=np.int64)

    def run():
        _lib.check(con.lib.kge_relation_prediction(ctypes.byref(con._desc), con._tab_ptrs, 0, count, out.ctypes.data, con._stream()),
                   con.lib)
        return out
    return run


def workload_a(d, reps):
    import torch
    from openkeonspark_amd import _lib
    con = make_config(d, False)
    L, st, n = con.lib, con._stream(), int(con.lib.getTestTotal())
    ids = torch.empty(2 * n, dtype=torch.int32, device=con.device)
    _lib.check(L.kge_test_entity_ids(0, n, ids.data_ptr(), st), L)
    query = con._tables[0].index_select(0, ids.long()).contiguous()
    counts = torch.empty((n, 4), dtype=torch.int64, device=con.device)

    def rows():
        _lib.check(L.kge_relation_prediction_rows(ctypes.byref(con._desc), con._tab_ptrs, query.data_ptr(), 0, n, counts.data_ptr(), st), L)
    ref = reference_counts(con, n)
    rows()
    want = ref().copy()
    equal = bool(np.array_equal(counts.cpu().numpy(), want))
    t_rows = timed(rows, reps)
    t_ref = timed(ref, reps)
    return dict(workload="a_fb15k237_rows", E=int(con.entTotal), R=int(con.relTotal), D=DIM, triples=n, rows_ms=t_rows * 1e3,
                relation_prediction_ms=t_ref * 1e3, ratio=t_rows / t_ref, counts_equal=equal)


def workload_b(d, reps):
    import torch
    import torch.distributed as dist
    from openkeonspark_amd import _lib, shard_eval
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29561")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        con = make_config(d, True)
        L, st, n, D = con.lib, con._stream(), int(con.lib.getTestTotal()), con.hidden_size
        per = max(1, int(con.lp_shard_query_bytes) // (2 * D * 4))
        want = reference_counts(con, n)().copy()       # one shard: this rank's table is the whole table
        got, _ = con.relation_prediction()
        equal = bool(np.array_equal(got, want))

        def exchange():
            for c0 in range(0, n, per):
                m = min(per, n - c0)
                ids = torch.empty(2 * m, dtype=torch.int32, device=con.device)
                _lib.check(L.kge_test_entity_ids(c0, m, ids.data_ptr(), st), L)
                shard_eval.query_rows(con, ids, 2 * m)
        t_all = timed(lambda: con.relation_prediction(), reps)
        t_ex = timed(exchange, reps)
        t_ref = timed(reference_counts(con, n), reps)
        return dict(workload="b_fb15k237_sharded_one_rank", E=int(con.entTotal), R=int(con.relTotal), D=DIM, triples=n,
                    rounds=-(-n // per), relation_prediction_sharded_ms=t_all * 1e3, exchange_ms=t_ex * 1e3,
                    exchange_share=t_ex / t_all, kge_relation_prediction_ms=t_ref * 1e3, counts_equal=equal)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dir", default=None, help="where the synthetic graph is written (default: a private temp dir, removed)")
    args = ap.parse_args()
    from openkeonspark_amd import synthetic
    base = args.dir or tempfile.mkdtemp(prefix="bench_relpred_shard_")
    try:
        d = synthetic.make_typed_dataset(os.path.join(base, "fb15k237_typed"), synthetic.FB15K237_TYPED)
        for w in args.which.split(","):
            if w == "a":
                print(json.dumps(workload_a(d, args.reps)), flush=True)
            elif w == "b":
                print(json.dumps(workload_b(d, args.reps)), flush=True)
    finally:
        if args.dir is None:
            shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
