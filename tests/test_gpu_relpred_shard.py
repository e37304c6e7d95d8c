"""Relation prediction with the entity rows supplied by the caller (kge_relation_prediction_rows) and the shard-aware
Config.relation_prediction / relation_prediction_distributed built on it: the rows path against kge_relation_prediction
exactly (every dimension bucket, the whole test set and a sub-range, a typed graph, many chunks) with a NaN-filled tables[0]
that must not be read, the argument checks, 2 and 4 gloo ranks against one process over the union table, errors that every
rank agrees on, and the driver's --mode test --test_relation 1 on a sharded checkpoint.

Every test first checks that the new entry point exists."""
import ctypes
import datetime
import functools
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from shard_rig import KG, finish_rank, load_ranks, run_worlds, start_rank, union_config
from shard_rig import make_config as rig_config

pytestmark = pytest.mark.gpu
OK, BAD_ARG, UNSUPPORTED = 0, -3, -4


def require_entry_point():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "kge_relation_prediction_rows"), "kge_relation_prediction_rows is not exported"
    return L


make_config = functools.partial(rig_config, relation=True)


def rows_counts(con, first, count):
    """kge_relation_prediction_rows over test triples [first, first+count), the h / t rows gathered from the whole table with
    torch and tables[0] replaced by a table of the same shape filled with NaN.  -> counts int64 [count, 4]."""
    import torch
    from openkeonspark_amd import _lib
    L = require_entry_point()
    st, dev = con._stream(), con.device
    ids = torch.empty(max(2 * count, 1), dtype=torch.int32, device=dev)
    _lib.check(L.kge_test_entity_ids(first, count, ids.data_ptr(), st), L)
    query = con._tables[0].index_select(0, ids[:2 * count].long()).contiguous()
    nan = torch.full_like(con._tables[0], float("nan"))
    ptrs = _lib.table_ptrs([nan.data_ptr()] + [t.data_ptr() for t in con._tables[1:]])
    counts = torch.full((max(count, 1), 4), -1, dtype=torch.int64, device=dev)
    _lib.check(L.kge_relation_prediction_rows(ctypes.byref(con._desc), ptrs, query.data_ptr(), first, count, counts.data_ptr(), st), L)
    return counts[:count].cpu().numpy()


def whole_table_counts(con, first, count):
    from openkeonspark_amd import _lib
    out = np.zeros((count, 4), dtype=np.int64)
    _lib.check(con.lib.kge_relation_prediction(ctypes.byref(con._desc), con._tab_ptrs, first, count, out.ctypes.data, con._stream()),
               con.lib)
    return out


@pytest.fixture(scope="module")
def typed_graph(tmp_path_factory):
    from openkeonspark_amd import synthetic
    return synthetic.make_typed_dataset(str(tmp_path_factory.mktemp("typed_relpred")), synthetic.SMALL_TYPED)


# ---------------------------------------------------------------------------------------------------------------------------
# 1-2: one process
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [16, 32, 64, 128, 200, 512, 1024])
def test_rows_path_equals_relation_prediction(typed_graph, dim):
    require_entry_point()
    con = make_config(dim, path=typed_graph)
    total = int(con.lib.getTestTotal())
    want = whole_table_counts(con, 0, total)
    assert want[:, 0].sum() > 0 and want[:, 2].sum() > 0 and (want[:, 1] < want[:, 0]).any()   # typed, filtered columns count
    assert np.array_equal(rows_counts(con, 0, total), want)
    assert np.array_equal(rows_counts(con, 37, 101), want[37:138])
    assert np.array_equal(rows_counts(con, total - 1, 1), want[total - 1:])


def test_many_chunks_give_the_same_counts(typed_graph):
    require_entry_point()
    con = make_config(200, path=typed_graph)
    total = int(con.lib.getTestTotal())
    want = whole_table_counts(con, 0, total)
    L = con.lib
    for budget in (1, 5 * con.relTotal * 4):       # one triple per chunk, five triples per chunk
        L.kge_set_option(b"relpred_chunk_bytes", budget)
        try:
            assert np.array_equal(rows_counts(con, 0, total), want), budget
            assert np.array_equal(rows_counts(con, 11, 23), want[11:34]), budget
        finally:
            L.kge_set_option(b"relpred_chunk_bytes", 256 << 20)
    assert np.array_equal(rows_counts(con, 0, total), want)


@pytest.mark.parametrize("model", ["TransH", "TransD", "TransR"])
def test_other_models_are_unsupported(model):
    import torch
    L = require_entry_point()
    con = make_config(16, model=model, scale=1.0)
    query = torch.zeros((4, 2, 16), dtype=torch.float32, device=con.device)
    counts = torch.empty((4, 4), dtype=torch.int64, device=con.device)
    rc = L.kge_relation_prediction_rows(ctypes.byref(con._desc), con._tab_ptrs, query.data_ptr(), 0, 4, counts.data_ptr(), con._stream())
    assert rc == UNSUPPORTED


def test_bad_ranges_are_refused_and_count_zero_checks_only():
    import torch
    L = require_entry_point()
    con = make_config(16, scale=1.0)
    total = int(con.lib.getTestTotal())
    query = torch.zeros((4, 2, 16), dtype=torch.float32, device=con.device)
    counts = torch.empty((4, 4), dtype=torch.int64, device=con.device)
    call = lambda first, count, q=query.data_ptr(), c=counts.data_ptr(): L.kge_relation_prediction_rows(
        ctypes.byref(con._desc), con._tab_ptrs, q, first, count, c, con._stream())
    assert call(total - 2, 4) == BAD_ARG
    assert call(total + 1, 0) == BAD_ARG
    assert call(-1, 2) == BAD_ARG
    assert call(0, -1) == BAD_ARG
    assert call(total, 0, None, None) == OK
    assert call(0, 0, None, None) == OK
    assert call(0, 4, None, None) == BAD_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# 3-4: ranks (gloo, one GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out_dir, data):
    import openkeonspark_amd as pkg
    con = start_rank(rank, world, port, data, relation=True, timeout=datetime.timedelta(seconds=60))
    total = int(con.lib.getTestTotal())
    out = {}
    out["all"], m_all = con.relation_prediction()
    out["part"], _ = con.relation_prediction(3, 10)
    out["one"], _ = con.relation_prediction(total - 1, 1)
    out["none"], _ = con.relation_prediction(5, 0)
    default_bytes = con.lp_shard_query_bytes
    con.lp_shard_query_bytes = 1 if rank != 1 else default_bytes     # one triple per round (the smallest value holds)
    out["rounds"], _ = con.relation_prediction()
    out["rounds_part"], _ = con.relation_prediction(2, 9)
    con.lp_shard_query_bytes = default_bytes
    m_dist = con.relation_prediction_distributed()
    # errors every rank agrees on: a range past the end on rank 0 only, then a different first on every rank
    raised = []
    for first, count in ((total - 2, 5) if rank == 0 else (0, 5), (rank, 5)):
        try:
            con.relation_prediction(first, count)
            raised.append(0)
        except pkg.KgeError:
            raised.append(1)
    out["raised"] = np.array(raised)
    out["after"], _ = con.relation_prediction(3, 10)        # a valid call still works afterwards
    finish_rank(con, out_dir, world, rank, metrics=json.dumps(dict(all=m_all, dist=m_dist)), **out)


@pytest.fixture(scope="module")
def sharded_runs(tmp_path_factory):
    require_entry_point()
    return run_worlds(_rank_worker, tmp_path_factory.mktemp("relpred_shard_ranks"), 35100 + os.getpid() % 1000)


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_equal_one_process_over_the_union_table(sharded_runs, world):
    base, data = sharded_runs
    zs = load_ranks(base, world)
    con = union_config(data, zs[0], relation=True)
    assert con.entTotal == 1003 and con.entTotal % world
    total = int(con.lib.getTestTotal())
    want, m_want = con.relation_prediction()
    assert want.shape == (total, 4) and want[:, 0].sum() > 0 and want[:, 2].sum() > 0
    for g, z in enumerate(zs):
        assert np.array_equal(z["ent"], zs[0]["ent"]) and np.array_equal(z["rel"], zs[0]["rel"])
        assert np.array_equal(z["all"], want), g
        assert np.array_equal(z["part"], want[3:13]), g
        assert np.array_equal(z["one"], want[total - 1:]), g
        assert z["none"].shape == (0, 4), g
        assert np.array_equal(z["rounds"], want), g
        assert np.array_equal(z["rounds_part"], want[2:11]), g
        assert np.array_equal(z["after"], want[3:13]), g
        m = json.loads(str(z["metrics"]))
        assert m["all"] == m_want and m["dist"] == m_want, g
        assert len(m_want) == 20


@pytest.mark.parametrize("world", [2, 4])
def test_bad_calls_raise_on_every_rank(sharded_runs, world):
    base, _ = sharded_runs
    for g, z in enumerate(load_ranks(base, world)):
        assert z["raised"].tolist() == [1, 1], g


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the driver
# ---------------------------------------------------------------------------------------------------------------------------
def _driver_worker(rank, world, port, out_dir, mode, run):
    sys.path.insert(0, ROOT)
    env = {"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world),
           "LOCAL_RANK": str(rank), "KGE_SINGLE_DEVICE": "1", "KGE_DIST_BACKEND": "gloo", "KGE_COUNTS_MIN_RECORDS": "0"}
    os.environ.update(env)
    from openkeonspark_amd import _lib
    from openkeonspark_amd import distribute_training as dt
    _lib.lib().kge_set_option(b"inv_table_max_bytes", 0)
    args = ["--input_path", KG, "--output_path", os.path.join(out_dir, run), "--embedding_dimension", "32",
            "--n_mini_batches", "5", "--ent_neg_rate", "3", "--alpha", "0.05", "--optimizer", "SGD", "--bern_flag", "1",
            "--train_times", "4", "--sparse_rows", "1", "--mode", mode, "--test_head", "1", "--test_relation", "1"]
    dt.main_fun(dt.parse_args(args))


def test_driver_mode_test_relation_on_a_sharded_checkpoint(tmp_path):
    require_entry_point()
    import shutil
    import torch.multiprocessing as mp
    port = 36100 + os.getpid() % 1000
    mp.start_processes(_driver_worker, args=(2, port, str(tmp_path), "train", "model"), nprocs=2, join=True, start_method="spawn")
    assert any(".shard" in f for f in os.listdir(str(tmp_path / "model")))
    results = {}
    for i, w in enumerate((2, 4, 1)):
        run = "test%d" % w
        shutil.copytree(str(tmp_path / "model"), str(tmp_path / run))
        mp.start_processes(_driver_worker, args=(w, port + 1 + i, str(tmp_path), "test", run), nprocs=w, join=True,
                           start_method="spawn")
        with open(str(tmp_path / run / "lp_results.json")) as f:
            results[w] = json.load(f)
    rel = [k for k in results[1] if k.startswith("rel")]
    assert len(rel) == 20 and len(results[1]) == 60
    for w in (2, 4):
        assert set(results[w]) == set(results[1]), w
        for k in rel:
            assert results[w][k] == results[1][k], (w, k)
    assert results[1]["rel_rank"] >= results[1]["rel_filter_rank"] >= 1.0
    n = 40   # test triples of kg_small: a near-tie flips one count of one triple, moving a metric by at most 1 / n
    for k in results[1]:
        if not k.startswith("rel"):
            assert abs(results[2][k] - results[1][k]) <= 2.0 / n + 1e-12, (k, results[2][k], results[1][k])
            assert results[2][k] == results[4][k], k
