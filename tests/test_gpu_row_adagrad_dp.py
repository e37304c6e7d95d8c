"""opt_method "RowAdagrad" across ranks (`gloo` ranks sharing the one GPU of the test box, tests/test_gpu_dp.py's rig; one spawn
per world -- the one-process runs made once for the module, then the worlds of 2 and 3 ranks one after another -- and the
one-rank RCCL rehearsal).  TransE on the sign-count path: the entity rows AND their accumulators -- one float per row -- are
sharded by row range (owner computes), the relation table and its accumulators stay replicated and are updated by every rank
from the all-reduced counts: integer sums, one kernel and one team shape, so the gathered table and the union of the ranks'
accumulator rows equal the one-process run bit for bit.  TransH: tables and accumulators replicated, the gathered float records
reduced in one order on every rank.  TransR: refused across ranks.  Every rank saves its accumulators beside its parameters as
`<var>/RowAdagrad`.  The rule itself: tests/test_gpu_row_adagrad.py."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_dp import _sharded_equals_one_process, _worker

pytestmark = pytest.mark.gpu

A0 = np.float32(0.1)
SLOT = "/RowAdagrad"


def _worker_with_accumulators(rank, world, port, out_dir, *args):
    """test_gpu_dp._worker, whose saved `get_parameters()` here also holds every accumulator as `<var>/RowAdagrad`, float32
    [rows]: whole where the table is replicated, gathered from the ranks' shards (a collective, like the parameter shards'
    gather) where the entity table is sharded."""
    sys.path.insert(0, ROOT)
    import torch
    import openkeonspark_amd as pkg
    from openkeonspark_amd.parallel import all_gather_chunks
    plain = pkg.Config.get_parameters

    def with_accumulators(con, mode="numpy"):
        res = plain(con, mode)
        for name, acc in zip(con.trainModel.table_names, con._rowadagrad_acc):
            if con._sharded(name):
                assert tuple(acc.shape) == (con._shard["chunk"],)      # shard-sized: one float per row this rank owns
                con.comm_fence("pg")
                full = torch.empty(con._shard["chunk"] * con.world_size, dtype=acc.dtype, device=acc.device)
                all_gather_chunks(full, acc, con._pg)
                acc = full[:con.entTotal]
            res[name + SLOT] = acc.detach().cpu().numpy()
        return res

    pkg.Config.get_parameters = with_accumulators
    _worker(rank, world, port, out_dir, *args)


def _spawn(tmp_path, world, port, *args):
    import torch.multiprocessing as mp
    mp.start_processes(_worker_with_accumulators, args=(world, port, str(tmp_path)) + args, nprocs=world, join=True, start_method="spawn")


def _load(tmp_path, world, suffix=""):
    res = [np.load(str(tmp_path / ("w%d_r%d%s.npz" % (world, r, suffix)))) for r in range(world)]
    for r in res:      # an accumulator per table, one float per row; they start at 0.1 and only grow, and some row was touched
        tables = [k for k in r.files if k not in ("losses", "states") and not k.endswith(SLOT)]
        assert "ent_embeddings" in tables and "rel_embeddings" in tables
        for k in tables:
            assert r[k + SLOT].shape == (r[k].shape[0],) and r[k + SLOT].dtype == np.float32, k
        acc = r["ent_embeddings" + SLOT]
        assert acc.min() >= A0 and acc.max() > A0
    return res


_PORT = [29600 + os.getpid() % 1000]


def _next_port():
    _PORT[0] += 1
    return _PORT[0]


@pytest.fixture(scope="module")
def one_process(tmp_path_factory):
    """The one-process runs the worlds below are compared with, made once: {model: (directory, result)}."""
    out = {}
    for model in ("TransE", "TransH"):
        d = tmp_path_factory.mktemp("row_adagrad_" + model)
        _spawn(d, 1, _next_port(), model, "RowAdagrad", True)
        out[model] = (d, _load(d, 1)[0])
        assert np.isfinite(out[model][1]["losses"]).all()
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_sharded_row_adagrad(one_process, world):
    """TransE, sparse rows, on 2 ranks and on 3 (kg_small's 1000 entities 334 / 334 / 332).  Every table -- the accumulators are
    saved as tables -- equals the one-process run bit for bit on every rank; the loss, summed over the ranks in another order, to
    rtol 2e-5."""
    d, one = one_process["TransE"]
    _spawn(d, world, _next_port(), "TransE", "RowAdagrad", True)
    _sharded_equals_one_process({1: [one], world: _load(d, world)}, world)


def test_one_rank_rccl_group_runs_the_sharded_step(one_process):
    """The one-rank RCCL group (`force_data_parallel`: the all-to-all exchanges on device memory, every collective a copy):
    tables, accumulators, losses and rng states equal the plain one-process run bit for bit."""
    d, plain = one_process["TransE"]
    _spawn(d, 1, _next_port(), "TransE", "RowAdagrad", True, False, 10, 0, True)
    rccl = _load(d, 1, "_rccl")[0]
    assert sorted(plain.files) == sorted(rccl.files)
    for k in plain.files:
        np.testing.assert_array_equal(plain[k], rccl[k], err_msg=k)


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_row_adagrad_from_gathered_records(one_process, world):
    """TransH: train_paths.records_step ending in kge_float_records_apply_rowadagrad on 2 ranks and on 3.  The replicas are
    bit-identical to each other; against one process (the same records in batch order) the per-row sums differ in fp32 order
    only -- held to tests/test_gpu_adagrad_dp.py's tolerance for the same comparison: 2e-4 of a table's largest element (the
    accumulators are tables here), losses to rtol 2e-5, rng states equal."""
    d, one = one_process["TransH"]
    _spawn(d, world, _next_port(), "TransH", "RowAdagrad", True)
    res = _load(d, world)
    for r in res:
        assert np.array_equal(r["states"], one["states"])
        assert np.allclose(r["losses"], one["losses"], rtol=2e-5, atol=0), (r["losses"], one["losses"])
        assert np.array_equal(r["losses"], res[0]["losses"])
    for k in one.files:
        if k in ("losses", "states"):
            continue
        for r in res[1:]:
            assert np.array_equal(res[0][k], r[k]), k
        ratio = float(np.abs(res[0][k] - one[k]).max() / np.abs(one[k]).max())
        print("row adagrad, %d ranks vs one process, %s: %.3g of the largest element (bound 2e-4)" % (world, k, ratio))
        assert ratio <= 2e-4, (k, ratio)


def test_transr_with_row_adagrad_is_refused_across_ranks(tmp_path):
    """TransR keeps dense gradient tables, and the data-parallel dense step cuts its flat buffer anywhere: every rank raises
    the KgeError that says so when it joins the world."""
    with pytest.raises(Exception, match="TransR with RowAdagrad is single-process only"):
        _spawn(tmp_path, 2, _next_port(), "TransR", "RowAdagrad")
