"""distribute_training with --shared_negatives_chunk under two `gloo` ranks (tests/test_gpu_dp.py's driver rig): an epoch on a
row-sharded entity table with Adagrad writes the per-rank shard files and a main file that records chunk and seed; one process
resumes that checkpoint, trains on, and ends where one uninterrupted process ends, bit for bit."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

CHUNK, SEED = 5, 77


def _driver_worker(rank, world, port, out_dir, run, train_times):
    sys.path.insert(0, ROOT)
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world),
                       "LOCAL_RANK": str(rank), "KGE_SINGLE_DEVICE": "1", "KGE_DIST_BACKEND": "gloo"})
    import torch.distributed as dist
    from openkeonspark_amd import distribute_training as dt
    if world > 1:      # gathering the sharded table afterwards is a collective: keep the process group beyond main_fun
        dist.init_process_group("gloo", rank=rank, world_size=world)
    args = ["--input_path", os.path.join(GOLDEN, "kg_small"), "--output_path", os.path.join(out_dir, run), "--embedding_dimension", "32",
            "--n_mini_batches", "7", "--ent_neg_rate", "3", "--alpha", "0.05", "--optimizer", "Adagrad", "--bern_flag", "1",
            "--train_times", str(train_times), "--work_threads", "4", "--shared_negatives_chunk", str(CHUNK),
            "--shared_negatives_seed", str(SEED)]
    con = dt.main_fun(dt.parse_args(args))
    assert con._shared_chunk == CHUNK and con._adagrad and con.batch_size % CHUNK != 0
    assert (world == 1) or (con._sharded("ent_embeddings") and con._tables[0].shape[0] == con._shard["chunk"])
    np.savez(os.path.join(out_dir, "%s_t%d_w%d_r%d.npz" % (run, train_times, world, rank)), step=con.global_step, **con.get_parameters())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_driver_on_two_ranks_then_a_one_process_resume(tmp_path):
    import torch.multiprocessing as mp
    port = 34300 + os.getpid() % 1000
    for i, (w, run, times) in enumerate(((2, "split", 1), (1, "split", 1), (1, "full", 2))):
        mp.start_processes(_driver_worker, args=(w, port + i, str(tmp_path), run, times), nprocs=w, join=True, start_method="spawn")
        if i == 0:
            files = set(os.listdir(str(tmp_path / "split")))
            assert {"model.ckpt-7.npz", "model.ckpt-7.shard0of2.npz", "model.ckpt-7.shard1of2.npz", "checkpoint"} <= files
            z = np.load(str(tmp_path / "split" / "model.ckpt-7.npz"))
            assert [int(x) for x in z["shared_negatives"]] == [CHUNK, SEED] and "ent_embeddings" not in z.files
            assert "adagrad" in np.load(str(tmp_path / "split" / "model.ckpt-7.shard1of2.npz")).files
    first = [np.load(str(tmp_path / ("split_t1_w2_r%d.npz" % g))) for g in range(2)]
    resumed, full = np.load(str(tmp_path / "split_t1_w1_r0.npz")), np.load(str(tmp_path / "full_t2_w1_r0.npz"))
    assert int(first[0]["step"]) == int(first[1]["step"]) == 7 and int(resumed["step"]) == int(full["step"]) == 14
    for k in ("ent_embeddings", "rel_embeddings"):
        assert np.array_equal(first[0][k], first[1][k]), k
        assert not np.array_equal(resumed[k], first[0][k]), k          # the resumed run trained on
        assert np.array_equal(resumed[k].view(np.uint32), full[k].view(np.uint32)), k
