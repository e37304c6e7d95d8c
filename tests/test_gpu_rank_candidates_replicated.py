"""Config.rank_candidates_distributed and validation_link_prediction_distributed(candidates=) on replicated tables: two gloo
ranks split the triples (per-triple lists are cut with them, a shared list is not), and every rank gets one process's counts and
metrics; a bad call on one rank raises on both and leaves none waiting."""
import os
import sys

import numpy as np
import pytest

from shard_rig import KG
from test_gpu_rank_candidates_dist import C, PG_TIMEOUT, ROOT, SEED, triples

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, out_dir, model):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=PG_TIMEOUT)
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(KG)
    con.set_work_threads(2)
    con.set_dimension(32)
    con.set_test_link_prediction(True)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    for t in con._tables:
        t.mul_(3.0)
    con.tables_changed()
    con.init_distributed()
    assert not con._sharded("ent_embeddings") and con.world_size == world
    tr = triples()
    h, t, r = tr[:, 0], tr[:, 1], tr[:, 2]
    rng = np.random.default_rng(3)
    lists = rng.integers(-1, con.entTotal + 2, (2, len(tr), C))          # a few pads and ids past the table among them
    shared = rng.integers(0, con.entTotal, C)
    same = True
    for kw in (dict(tail_candidates=lists[0], head_candidates=lists[1]), dict(tail_candidates=shared, head_candidates=lists[1], filtered=False),
               dict(head_candidates=shared), dict(tail_candidates=lists[0][:1])):
        part = (h[:1], t[:1], r[:1]) if len(kw.get("tail_candidates", lists[0])) == 1 else (h, t, r)
        got, met = con.rank_candidates_distributed(*part, **kw)
        want, want_met = con.rank_candidates(*part, **kw)                # this rank's own whole tables
        same = same and np.array_equal(got, want) and met == want_met and bool(want.any())
    for kw in (dict(candidates=C, seed=SEED), dict(candidates=C, seed=SEED, sample=7, test_head=False, type_constrained=True)):
        got, met = con.validation_link_prediction_distributed(**kw)
        want, want_met = con.validation_link_prediction(**kw)
        same = same and np.array_equal(got, want) and met == want_met and bool(want.any())
    raised = []
    for call in (lambda: con.rank_candidates_distributed(h, t, r, lists[0][:, :C - (rank == 0)], None),
                 lambda: con.rank_candidates_distributed([con.entTotal if rank == world - 1 else 0], [1], [0], shared),
                 lambda: con.validation_link_prediction_distributed(candidates=-1 if rank == world - 1 else C)):
        try:
            call()
            raised.append(0)
        except pkg.KgeError:
            raised.append(1)
    after, _ = con.rank_candidates_distributed(h[:3], t[:3], r[:3], shared)
    same = same and np.array_equal(after, con.rank_candidates(h[:3], t[:3], r[:3], shared)[0])
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), raised=np.array(raised), same=same)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_give_one_process_counts(tmp_path):
    import torch.multiprocessing as mp
    from openkeonspark_amd.Config import Config
    assert hasattr(Config, "rank_candidates_distributed"), "Config.rank_candidates_distributed is missing"
    mp.start_processes(_worker, args=(2, 42700 + os.getpid() % 600, str(tmp_path), "TransH"), nprocs=2, join=True, start_method="spawn")
    for g in range(2):
        z = np.load(os.path.join(str(tmp_path), "r%d.npz" % g))
        assert bool(z["same"]) and z["raised"].tolist() == [1, 1, 1], g
