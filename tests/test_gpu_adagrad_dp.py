"""opt_method "Adagrad" across ranks (`gloo` ranks sharing the one GPU of the test box, tests/test_gpu_dp.py's rig, at most 8
ranks at a time).  TransE on the sign-count path: the entity rows AND their accumulator rows are sharded by row range (owner
computes), the relation table and its accumulator stay replicated and are updated by every rank from the all-reduced counts --
integer sums and one per-row update function, so every table equals the one-process run bit for bit.  TransH / TransD: tables
and accumulators replicated, the gathered float records reduced in one order on every rank.  TransR: refused across ranks.
Every rank saves its ACCUMULATORS beside its parameters (`<var>/Adagrad`, the shards of a sharded one gathered as the parameter
shards are), so each comparison below holds the accumulators to what it asks of the tables.  The rule itself:
tests/test_gpu_adagrad.py."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_dp import _sharded_equals_one_process, _worker

pytestmark = pytest.mark.gpu


def _worker_with_accumulators(rank, world, port, out_dir, *args):
    """test_gpu_dp._worker, whose saved `get_parameters()` here also holds every accumulator table as `<var>/Adagrad`: whole
    where the table is replicated, gathered from the ranks' shards (a collective, like the parameter shards' gather) where the
    entity table is sharded."""
    sys.path.insert(0, ROOT)
    import torch
    import openkeonspark_amd as pkg
    from openkeonspark_amd.parallel import all_gather_chunks
    plain = pkg.Config.get_parameters

    def with_accumulators(con, mode="numpy"):
        res = plain(con, mode)
        for name, acc in zip(con.trainModel.table_names, con._adagrad_acc):
            if con._sharded(name):
                assert tuple(acc.shape) == (con._shard["chunk"], con.hidden_size)     # shard-sized, not a whole table
                con.comm_fence("pg")
                full = torch.empty((con._shard["chunk"] * con.world_size, acc.shape[1]), dtype=acc.dtype, device=acc.device)
                all_gather_chunks(full.view(-1), acc.reshape(-1), con._pg)
                acc = full[:con.entTotal]
            res[name + "/Adagrad"] = acc.detach().cpu().numpy()
        return res

    pkg.Config.get_parameters = with_accumulators
    _worker(rank, world, port, out_dir, *args)


def _run_worlds(tmp_path, worlds, *args):
    """test_gpu_dp._run_worlds with the worker above; every result must hold an accumulator per table, and one that moved."""
    import torch.multiprocessing as mp
    port = 29600 + os.getpid() % 1000
    for i, w in enumerate(worlds):
        mp.start_processes(_worker_with_accumulators, args=(w, port + i, str(tmp_path)) + args, nprocs=w, join=True, start_method="spawn")
    res = {w: [np.load(str(tmp_path / ("w%d_r%d.npz" % (w, r)))) for r in range(w)] for w in worlds}
    for w in worlds:
        for r in res[w]:
            tables = [k for k in r.files if k not in ("losses", "states") and not k.endswith("/Adagrad")]
            for k in tables:
                assert r[k + "/Adagrad"].shape == r[k].shape, k
            acc = r["ent_embeddings/Adagrad"]
            assert acc.min() >= np.float32(0.1) and acc.max() > np.float32(0.1)        # starts at 0.1 and only grows; some row was touched
    return res


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_sharded_adagrad(tmp_path, world):
    res = _run_worlds(tmp_path, [1, world], "TransE", "Adagrad", True)
    _sharded_equals_one_process(res, world)
    assert np.isfinite(res[1][0]["losses"]).all()


def test_ranks_sharded_adagrad_with_an_empty_shard(tmp_path):
    """33 entities on 8 ranks (test_gpu_dp.test_ranks_sharded_with_an_empty_shard's data): rank 7 owns no row and no accumulator
    row, joins every collective and applies the relation update like everyone else."""
    from openkeonspark_amd import parallel, synthetic
    E, R, n = 33, 5, 400
    assert parallel.chunk_size(E, 8) == 5 and 7 * 5 >= E > 6 * 5
    rng = np.random.default_rng(33)
    data = synthetic.write_openke_dir(str(tmp_path / "kg33"), E, R, rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n))
    res = _run_worlds(tmp_path, [1, 8], "TransE", "Adagrad", True, False, 10, 0, False, data)
    _sharded_equals_one_process(res, 8)


def test_ranks_sharded_adagrad_with_relation_negatives(tmp_path):
    """ent_neg_rate 2, rel_neg_rate 2, dim 48 on 2 ranks: relation rows take records from relation-corrupted negatives too.  All
    relation rows are listed with their all-reduced counts and no live mask: a relation whose counts are zero has zero gradient
    and keeps its row and accumulator, as in one process, where it is not listed at all."""
    res = _run_worlds(tmp_path, [1, 2], "TransE", "Adagrad", True, False, 10, 0, False, None, 48, 2, 2)
    _sharded_equals_one_process(res, 2)


@pytest.mark.parametrize("model_name", ["TransH", "TransD"])
def test_ranks_adagrad_from_gathered_records(tmp_path, model_name):
    """train_paths.records_step ending in kge_float_records_apply_adagrad on 2 ranks: the replicas are bit-identical to each other;
    against one process (the same records in batch order) the per-row sums differ in fp32 order only -- held to the tolerance
    tests/test_gpu_lazy_rows_dp.py applies to LazyAdam for the same comparison: 2e-4 of a table's largest element, losses to
    rtol 2e-5, rng states equal."""
    res = _run_worlds(tmp_path, [1, 2], model_name, "Adagrad", True)
    one = res[1][0]
    for r in res[2]:
        assert np.array_equal(r["states"], one["states"])
        assert np.allclose(r["losses"], one["losses"], rtol=2e-5, atol=0), (r["losses"], one["losses"])
        assert np.array_equal(r["losses"], res[2][0]["losses"])
    for k in one.files:
        if k in ("losses", "states"):
            continue
        assert np.array_equal(res[2][0][k], res[2][1][k]), k
        ratio = float(np.abs(res[2][0][k] - one[k]).max() / np.abs(one[k]).max())
        print("adagrad ranks vs one process, %s %s: %.3g of the largest element (bound 2e-4)" % (model_name, k, ratio))
        assert ratio <= 2e-4, (k, ratio)


def test_transr_with_adagrad_is_refused_across_ranks(tmp_path):
    """TransR keeps dense gradient tables; the data-parallel dense step has no flat accumulator for its exchange: every rank
    raises the KgeError that says so when it joins the world."""
    with pytest.raises(Exception, match="TransR with Adagrad is single-process only"):
        _run_worlds(tmp_path, [2], "TransR", "Adagrad")
