"""Config.rank_triples_sampled_distributed on replicated tables: two gloo ranks split the triples, the hash stays indexed by
the global triple index, and every rank gets one process's counts; a bad call raises on every rank and leaves none waiting."""
import datetime
import os
import sys

import numpy as np
import pytest

from shard_rig import KG, make_config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG_TIMEOUT = datetime.timedelta(seconds=60)
C, SEED = 21, 77


def split(path, name):
    """The triples of a split file as int64 [n, 3] (h, t, r), file order."""
    with open(os.path.join(path, name + "2id.txt")) as f:
        tok = f.read().split()
    return np.asarray(tok[1:1 + 3 * int(tok[0])], dtype=np.int64).reshape(-1, 3)


def triples():
    va = split(KG, "valid")
    return np.concatenate([va, split(KG, "test")[:1], va[:4]])      # an odd number: the ranks' slices differ in length


def _worker(rank, world, port, out_dir, model):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=PG_TIMEOUT)
    import openkeonspark_amd as pkg
    con = pkg.Config()               # make_config's tables (the same seed, the same scale), with a work thread per rank
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
    res = {}
    for name, part, kw in (("odd", tr, {}), ("one", tr[:1], {}), ("none", tr[:0], {}), ("tail_typed", tr[:9], dict(test_head=False, type_constrained=True)),
                           ("raw", tr[:9], dict(filtered=False))):
        got, met = con.rank_triples_sampled_distributed(part[:, 0], part[:, 1], part[:, 2], C, seed=SEED, **kw)
        want, want_met = con.rank_triples_sampled(part[:, 0], part[:, 1], part[:, 2], C, seed=SEED, **kw)      # this rank's own whole tables
        res[name], res[name + "_local"] = got, want
        assert met == want_met, name
    raised = 0
    try:
        con.rank_triples_sampled_distributed([con.entTotal if rank == world - 1 else 0], [1], [0], C)
    except pkg.KgeError:
        raised = 1
    res["after"], _ = con.rank_triples_sampled_distributed(tr[:3, 0], tr[:3, 1], tr[:3, 2], C, seed=SEED)
    np.savez(os.path.join(out_dir, "%s_r%d.npz" % (model, rank)), raised=raised, **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_give_one_process_counts(tmp_path):
    import torch.multiprocessing as mp
    model = "TransH"
    mp.start_processes(_worker, args=(2, 39300 + os.getpid() % 600, str(tmp_path), model), nprocs=2, join=True, start_method="spawn")
    con = make_config(32, model=model)
    tr = triples()
    assert len(tr) % 2 == 1
    one = lambda part, **kw: con.rank_triples_sampled(part[:, 0], part[:, 1], part[:, 2], C, seed=SEED, **kw)[0]
    want = {"odd": one(tr), "one": one(tr[:1]), "none": np.zeros((0, 2, 2), np.int64), "tail_typed": one(tr[:9], test_head=False, type_constrained=True),
            "raw": one(tr[:9], filtered=False), "after": one(tr[:3])}
    assert want["odd"][:, :, 0].any() and want["odd"][:, 1].any() and not want["tail_typed"][:, 1].any()
    for g in range(2):
        z = np.load(os.path.join(str(tmp_path), "%s_r%d.npz" % (model, g)))
        for k, w in want.items():
            assert z[k].shape == w.shape and np.array_equal(z[k], w), (g, k)
            if k + "_local" in z:
                assert np.array_equal(z[k + "_local"], w), (g, k)
        assert int(z["raised"]) == 1
