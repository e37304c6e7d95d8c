"""opt_method "RowAdagrad" through the training driver and its checkpoints: interrupt and resume in one process (TransE on the
sign-count path, TransH from float records), a row-sharded checkpoint written on 2 ranks and resumed on 1 and on 3, and new
entities (accumulators of the initial value on every rank).  The accumulators are saved as `<var>/RowAdagrad`, float32 [rows],
and as `rowadagrad` in the shard files.  Rigs: tests/test_driver.py and tests/test_gpu_shard_checkpoint.py (`gloo` ranks on the
one GPU of the test box; every comparison bit for bit -- the sharded step equals one process's,
tests/test_gpu_row_adagrad_dp.py).  The files alone, and checkpoints that cross optimizers: tests/test_row_adagrad_plan.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from openkeonspark_amd import distribute_training as dt
from test_gpu_shard_checkpoint import DIM, E_NEW, E_OLD, _copy, _driver_worker, _grown_dataset, _rank_env, _spawn

pytestmark = pytest.mark.gpu

A0 = np.float32(0.1)
OPT = "RowAdagrad"


@pytest.mark.parametrize("model", ["TransE", "TransH"])
def test_driver_checkpoint_resume_is_bit_identical(tmp_path, model, monkeypatch):
    """tests/test_gpu_adagrad_checkpoint.py's construction: four epochs in one go equal two plus a resumed two in every table
    AND every accumulator; the checkpoint holds `<var>/RowAdagrad`, one float per row, for every table, and neither Adam's
    scalars nor Adagrad's tables."""
    from openkeonspark_amd import _lib
    monkeypatch.setenv("KGE_COUNTS_MIN_RECORDS", "0")
    out = str(tmp_path / "run")
    base = ["--input_path", os.path.join(GOLDEN, "kg_small"), "--output_path", out, "--embedding_dimension", "32",
            "--n_mini_batches", "5", "--ent_neg_rate", "3", "--alpha", "0.05", "--optimizer", OPT, "--bern_flag", "1",
            "--model", model]
    fresh = lambda: _lib.lib().kge_set_option(b"libc_rand_restart", 1)   # each run below stands for a new process
    fresh()
    full = dt.main_fun(dt.parse_args(base + ["--train_times", "4", "--output_path", str(tmp_path / "full")]))
    assert full._row_adagrad and not full._adagrad and full._grads == []
    want = full.get_parameters()
    fresh()
    a = dt.main_fun(dt.parse_args(base + ["--train_times", "2"]))
    assert dt.get_last_step(out) == 10 and a.global_step == 10
    z = np.load(os.path.join(out, "model.ckpt-10.npz"))
    for name in a.trainModel.table_names:
        acc = z[name + "__RowAdagrad"]
        assert acc.shape == (z[name].shape[0],) and acc.dtype == np.float32 and acc.min() >= A0 and acc.max() > A0, name
    assert "beta1_power" not in z.files and not any(k.endswith(("__Adam", "__Adagrad")) for k in z.files)
    fresh()
    b = dt.main_fun(dt.parse_args(base + ["--train_times", "2"]))
    assert b.global_step == 20 and dt.get_last_step(out) == 20
    got = b.get_parameters()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for x, y in zip(full._rowadagrad_acc, b._rowadagrad_acc):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())


def _final_checkpoint(run_dir):
    """The checkpoint the `checkpoint` pointer names, the entity rows and accumulators of a sharded one assembled."""
    base = os.path.join(run_dir, "model.ckpt-%d" % dt.get_last_step(run_dir))
    z = {k.replace("__", "/"): v for k, v in np.load(base + ".npz").items()}
    if "ent_embeddings" not in z:
        parts = dt.shard_files(base, ("rows", "rowadagrad"))
        z["ent_embeddings"] = dt.read_entity_rows(base, 0, parts[1], DIM, "rows", parts)[0]
        z["ent_embeddings/RowAdagrad"] = dt.read_entity_rows(base, 0, parts[1], None, "rowadagrad", parts)[0]
    return z


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """4 uninterrupted epochs on 2 ranks, and the checkpoint of 2 epochs on 2 ranks (kept pristine: each test resumes a copy)."""
    d = tmp_path_factory.mktemp("shard_ckpt_row_adagrad")
    _spawn(_driver_worker, 2, str(d / "full"), 4, OPT, str(d / "full"))
    _spawn(_driver_worker, 2, str(d / "ckpt10"), 2, OPT, str(d / "ckpt10"))
    assert dt.get_last_step(str(d / "ckpt10")) == 10
    return d


def test_shard_files_hold_the_accumulator_rows(runs):
    ckpt = str(runs / "ckpt10")
    for g in range(2):
        with np.load(os.path.join(ckpt, "model.ckpt-10.shard%dof2.npz" % g)) as z:
            assert sorted(z.files) == ["ent_total", "hi", "lo", "rowadagrad", "rows"]
            assert z["rows"].shape == (500, DIM) and z["rowadagrad"].shape == (500,) and z["rowadagrad"].dtype == np.float32
            assert z["rowadagrad"].min() >= A0 and z["rowadagrad"].max() > A0
    with np.load(os.path.join(ckpt, "model.ckpt-10.npz")) as z:     # replicated state only
        assert not any(k.startswith("ent_embeddings") for k in z.files) and z["rel_embeddings__RowAdagrad"].shape == (z["rel_embeddings"].shape[0],)


@pytest.mark.parametrize("world", [1, 3])
def test_sharded_checkpoint_resumes_at_another_size(runs, tmp_path, world):
    """The 2-rank checkpoint resumed in one process and on 3 ranks ends as the uninterrupted 2-rank run: tables, accumulators
    (from the final checkpoints, assembled), global_step and rng streams."""
    run = _copy(runs / "ckpt10", tmp_path / "run")
    _spawn(_driver_worker, world, run, 2, OPT, str(tmp_path / "resumed"))
    want, got = np.load(str(runs / "full") + "_r0.npz"), np.load(str(tmp_path / "resumed") + "_r0.npz")
    assert int(got["step"]) == int(want["step"]) == 20 and sorted(got.files) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k
    cw, cg = _final_checkpoint(str(runs / "full")), _final_checkpoint(run)
    assert sorted(cg) == sorted(cw) and "ent_embeddings/RowAdagrad" in cw and "rel_embeddings/RowAdagrad" in cw
    for k in cw:
        assert np.array_equal(cg[k], cw[k]), k


def _restore_and_step(world, data_dir, ckpt, opt):
    """restore_checkpoint of `ckpt` over the dataset `data_dir` under optimizer `opt`, then 2 steps.  -> the gathered tables
    before and after the steps and, under RowAdagrad, this rank's accumulators of rows [lo, hi) right after the restore."""
    import torch
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(data_dir)
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(DIM); con.set_nbatches(5)
    con.set_ent_neg_rate(3); con.set_alpha(0.01); con.set_opt_method(opt)
    con.sparse_rows = True
    con.counts_min_records = 0
    con.init()
    con.set_model_and_session(pkg.TransE)
    if world > 1:
        con.init_distributed()
    dt.restore_checkpoint(con, ckpt)
    before = con.get_parameters()
    lo, hi = (con._shard["lo"], con._shard["hi"]) if world > 1 else (0, con.entTotal)
    acc = {}
    if getattr(con, "_row_adagrad", False):
        acc = dict(acc=con._rowadagrad_acc[0][:hi - lo].cpu().numpy(), rel_acc=con._rowadagrad_acc[1].cpu().numpy())
    for _ in range(2):
        con.train_step()
    after = con.get_parameters()
    torch.cuda.synchronize()
    return dict(lo=lo, hi=hi, step=con.global_step, **acc, **{"before_" + k: v for k, v in before.items()},
                **{"after_" + k: v for k, v in after.items()})


def _grow_worker(rank, world, port, data_dir, ckpt, opt, result):
    dist = _rank_env(rank, world, port)
    np.savez("%s_r%d.npz" % (result, rank), **_restore_and_step(world, data_dir, ckpt, opt))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture
def one_process():
    """The settings a rank of the rigs runs under (_rank_env), for the one-process side done in the test's own process."""
    from openkeonspark_amd import _lib
    L = _lib.lib()
    L.kge_set_option(b"inv_table_max_bytes", 0)      # norms from the rows themselves, as the sharded step's gathered rows give them
    L.kge_set_option(b"libc_rand_restart", 1)
    yield lambda data_dir, ckpt, opt: _restore_and_step(1, data_dir, ckpt, opt)
    L.kge_set_option(b"inv_table_max_bytes", 256 << 20)


def test_sharded_checkpoint_grows_new_entities(runs, tmp_path, one_process):
    """The 2-rank checkpoint of 1000 entities resumed on 2 ranks over 2100: the accumulators of the new entities hold the initial
    value on every rank (zeros, as Adam's slots get, would divide by zero at their first gradient), the old rows keep theirs,
    the new parameter rows are one process's draw, and two steps later every table still equals one process's."""
    ckpt = os.path.join(str(runs / "ckpt10"), "model.ckpt-10.npz")
    data = _grown_dataset(str(tmp_path / "grown"))
    one = one_process(data, ckpt, OPT)
    _spawn(_grow_worker, 2, data, ckpt, OPT, str(tmp_path / "two"))
    two = [np.load(str(tmp_path / ("two_r%d.npz" % g))) for g in range(2)]
    z = _final_checkpoint(str(runs / "ckpt10"))
    assert [(int(t["lo"]), int(t["hi"])) for t in two] == [(0, 1050), (1050, 2100)]
    ent = one["before_ent_embeddings"]
    grown = dt.grow_table(z["ent_embeddings"], E_NEW, np.random.default_rng(0 + 1))   # one process's draw, by hand
    assert ent.shape == (E_NEW, DIM) and np.array_equal(ent, grown) and np.abs(ent[E_OLD:]).max() > 0
    for t in two:
        assert int(t["step"]) == int(one["step"]) == 12
        for k in one:
            if k.startswith(("before_", "after_")):
                assert np.array_equal(t[k], one[k]), k
        assert np.array_equal(t["rel_acc"], z["rel_embeddings/RowAdagrad"])
    acc = np.concatenate([t["acc"] for t in two])
    assert acc.shape == (E_NEW,) and np.array_equal(acc, one["acc"]) and np.array_equal(acc[:E_OLD], z["ent_embeddings/RowAdagrad"])
    assert (acc[E_OLD:] == A0).all() and (two[1]["acc"] == A0).all() and acc[:E_OLD].max() > A0
    assert np.isfinite(one["after_ent_embeddings"]).all()
    assert (one["after_ent_embeddings"][E_OLD:] != ent[E_OLD:]).any()               # new entities trained, from finite steps


def test_checkpoints_that_cross_optimizers(runs, tmp_path, one_process, monkeypatch):
    """A checkpoint without per-row accumulators (one process, Adagrad) resumes under RowAdagrad with fresh ones; the sharded
    RowAdagrad checkpoint restored into an SGD session takes the tables from the shard files, ignores the accumulators, and
    trains on."""
    monkeypatch.setenv("KGE_COUNTS_MIN_RECORDS", "0")
    run = str(tmp_path / "adagrad")
    data = os.path.join(GOLDEN, "kg_small")
    old = dt.main_fun(dt.parse_args(["--input_path", data, "--output_path", run, "--embedding_dimension", str(DIM), "--n_mini_batches", "5",
                                     "--ent_neg_rate", "3", "--alpha", "0.01", "--optimizer", "Adagrad", "--bern_flag", "1",
                                     "--train_times", "1", "--sparse_rows", "1"])).get_parameters()
    ckpt = os.path.join(run, "model.ckpt-5.npz")
    with np.load(ckpt) as z:
        assert "ent_embeddings__Adagrad" in z.files and not any("RowAdagrad" in k for k in z.files)
    one = one_process(data, ckpt, OPT)
    assert np.array_equal(one["before_ent_embeddings"], old["ent_embeddings"]) and int(one["step"]) == 7
    assert one["acc"].shape == (1000,) and (one["acc"] == A0).all() and (one["rel_acc"] == A0).all()
    assert np.isfinite(one["after_ent_embeddings"]).all() and (one["after_ent_embeddings"] != old["ent_embeddings"]).any()
    back = one_process(data, os.path.join(str(runs / "ckpt10"), "model.ckpt-10.npz"), "SGD")
    z = _final_checkpoint(str(runs / "ckpt10"))
    assert np.array_equal(back["before_ent_embeddings"], z["ent_embeddings"]) and int(back["step"]) == 12 and "acc" not in back
    assert np.array_equal(back["before_rel_embeddings"], z["rel_embeddings"])
    assert np.isfinite(back["after_ent_embeddings"]).all() and (back["after_ent_embeddings"] != z["ent_embeddings"]).any()
