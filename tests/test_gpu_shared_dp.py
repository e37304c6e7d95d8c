"""Shared negatives on a row-sharded entity table across ranks (train_paths.shared_sharded_step): `gloo` ranks sharing the one GPU
of the test box, as in tests/test_gpu_dp.py, against the one-process shared step of the same global batch.

Chunks are chunks of the GLOBAL batch position and the candidates and sides hashes of it, the gradients integer sign counts: the
union of the shards equals the one-process tables bit for bit at any rank count, with the optimizer's slot rows; only the loss is
summed in another order.  TransE, D = 48, 8 sampler threads, Bernoulli, P = 5, N = 3; the batch (857 of the 1003-entity graph's
6000 triples) is no multiple of P, so the slice bounds of every world cut chunks.

One spawn per world runs all of that world's jobs (a process start and a HIP start cost more than the steps); the fixture `runs`
does them once, the tests read what the ranks wrote."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

P, N, SEED, DIM = 5, 3, 20240, 48
OPTS = ("SGD", "LazyAdam", "Adagrad")
NB_MAIN, NB_FIVE, NB_E33 = 7, 1200, 7        # batches of 857, 5 and 57 positives
CKPT_OPT = "LazyAdam"                        # the checkpointed run: rows, two moment rows, beta powers


def _config(pkg, data, opt, nbatches, dim=DIM, chunk=P, seed=SEED):
    pkg._lib.lib().kge_set_option(b"libc_rand_restart", 1)      # every Config starts as in a fresh process
    con = pkg.Config()
    con.set_in_path(data)
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(dim); con.set_nbatches(nbatches)
    con.set_ent_neg_rate(N); con.set_rel_neg_rate(0); con.set_alpha(0.02); con.set_opt_method(opt)
    con.sparse_rows = True
    con.set_shared_negatives(chunk, seed=seed)
    con.init()
    return con


def _state(con, losses):
    """Losses, rng streams, the gathered tables (collective) and this rank's rows [lo, hi) of the entity slot tables."""
    out = dict(losses=np.array(losses, dtype=np.float64), states=con.get_stream_states(), **con.get_parameters())
    lo, hi = (con._shard["lo"], con._shard["hi"]) if con._sharded("ent_embeddings") else (0, con.entTotal)
    slots = dict(m=con._adam_m, v=con._adam_v) if con._lazy_adam else (dict(a=con._adagrad_acc) if con._adagrad else {})
    for k, tabs in slots.items():
        out[k + "_ent"], out[k + "_rel"] = tabs[0][:hi - lo].cpu().numpy(), tabs[1].cpu().numpy()
    out["lo"], out["hi"] = np.int64(lo), np.int64(hi)
    return out


def _traffic(con, step):
    """[n_pos, n_chunks, ids outside the table, rows requested, rows served, records sent, records received, entity-side keys >= 0]
    of the step just trained, from the step's own lists and Config.last_exchange_sizes()."""
    b = con._sparse_buf
    n_pos, n_chunks = b["shared_shape"]
    cand, pair = con.shared_negatives_of(step)
    assert cand.shape == (n_chunks, N) and pair.shape == (n_pos, N)
    pos = b["shared_batch"].cpu().numpy()[:, :n_pos]
    ids = np.concatenate([pos[0], pos[1], cand.reshape(-1)])
    outside = int(((ids < 0) | (ids >= con.entTotal)).sum())
    dst = b["dst"][:3 * n_pos + n_chunks * N].cpu().numpy()
    keyed = int((np.concatenate([dst[:2 * n_pos], dst[3 * n_pos:]]) >= 0).sum())
    s = con.last_exchange_sizes()
    return [n_pos, n_chunks, outside, s["rows_requested"], s["rows_served"], s["records_sent"], s["records_received"], keyed]


def _train(pkg, con, out_dir, tag, steps, dumps, dist_on, ckpt_dir=None, ckpt_at=None, resume=None):
    from openkeonspark_amd import distribute_training as dt
    con.set_model_and_session(pkg.TransE)
    assert con.batch_size % P != 0 or con.batch_size == P
    if dist_on:
        if dist_on == "rccl":
            con.force_data_parallel = True
        con.init_distributed()
        assert con._sharded("ent_embeddings") and con._tables[0].shape[0] == con._shard["chunk"]
    if resume:
        assert dt.restore_checkpoint(con, resume) == 2
    losses, traffic = [], []
    for _ in range(steps):
        step = con.global_step
        losses.append(con.train_step())
        if dist_on:
            traffic.append(_traffic(con, step))
        if con.global_step in dumps:
            np.savez(os.path.join(out_dir, "%s_s%d_w%d_r%d.npz" % (tag, con.global_step, con.world_size if dist_on != "rccl" else 0, con.rank)),
                     traffic=np.array(traffic, dtype=np.int64).reshape(-1, 8), first_pos=np.int64(con._first_pos),
                     batch=np.int64(con.batch_size), **_state(con, losses))
        if ckpt_at == con.global_step:
            dt.save_checkpoint(con, ckpt_dir, write=con.rank == 0)
    return con


def _refused(fn, said):
    from openkeonspark_amd import KgeError
    try:
        fn()
    except KgeError as exc:
        return str(exc)
    return "NOT REFUSED: " + said


def _worker(rank, world, port, out_dir, data, data33, rccl):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    elif rccl:       # a ONE-rank RCCL group with force_data_parallel: the step's own machinery on device memory
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    import openkeonspark_amd as pkg
    from openkeonspark_amd import distribute_training as dt
    dist_on = "rccl" if rccl else world > 1
    ckpt_dir = os.path.join(out_dir, "ckpt")
    ckpt = os.path.join(ckpt_dir, "model.ckpt-2.npz")
    refusals = {}
    if world in (1, 2, 3, 4):
        for opt in OPTS:
            save = world == 2 and opt == CKPT_OPT
            con = _train(pkg, _config(pkg, data, opt, NB_MAIN), out_dir, "main_" + opt, 4 if world == 1 and not rccl else 3, (3, 4), dist_on,
                         ckpt_dir if save else None, 2 if save else None)
            if opt == "SGD":
                refusals["persistent"] = _refused(lambda: con.train_steps(2, persistent=True), "train_steps(persistent=True)")
    if world in (1, 4) and not rccl:
        _train(pkg, _config(pkg, data, "SGD", NB_FIVE), out_dir, "five", 3, (3,), dist_on)          # 5 positives on 8 threads: empty slices
        _train(pkg, _config(pkg, data, CKPT_OPT, NB_MAIN), out_dir, "resumed", 2, (4,), dist_on, resume=ckpt)
    if world in (1, 8) and not rccl:
        for opt in ("SGD", "LazyAdam"):
            _train(pkg, _config(pkg, data33, opt, NB_E33), out_dir, "e33_" + opt, 3, (3,), dist_on)   # 33 entities: the last shard is empty
    if world == 2:
        for name, kw in (("resume_chunk", dict(chunk=4)), ("resume_seed", dict(seed=SEED + 1))):
            bad = _config(pkg, data, CKPT_OPT, NB_MAIN, **kw)
            bad.set_model_and_session(pkg.TransE)
            bad.init_distributed()
            refusals[name] = _refused(lambda: dt.restore_checkpoint(bad, ckpt), name)
        wide = _config(pkg, data, "SGD", NB_MAIN, dim=50)
        wide.set_model_and_session(pkg.TransE)
        refusals["width"] = _refused(wide.init_distributed, "width 50 on 2 ranks")

        def typed():
            c = pkg.Config()
            c.set_type_constrained_sampling(True)
            c.set_shared_negatives(P)
        refusals["typed"] = _refused(typed, "typed sampling")
    with open(os.path.join(out_dir, "refusals_w%d_r%d%s.json" % (world, rank, "_rccl" if rccl else "")), "w") as f:
        json.dump(refusals, f)
    torch.cuda.synchronize()
    if world > 1 or rccl:
        dist.barrier()
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import torch.multiprocessing as mp
    from openkeonspark_amd import parallel, synthetic
    base = tmp_path_factory.mktemp("shared_dp")
    data = synthetic.make_typed_dataset(str(base / "kg1003"), synthetic.SMALL_TYPED, entities=1003, train=6000, valid=100, test=60)
    E, R, n = 33, 5, 400
    assert parallel.chunk_size(E, 8) == 5 and 7 * 5 >= E > 6 * 5
    rng = np.random.default_rng(33)
    data33 = synthetic.write_openke_dir(str(base / "kg33"), E, R, rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n))
    port = 33100 + os.getpid() % 1000
    # (2 ranks first: they write the checkpoint the other worlds resume; one world after another, at most 8 ranks at once)
    for i, (w, rccl) in enumerate(((2, False), (1, False), (3, False), (4, False), (8, False), (1, True))):
        mp.start_processes(_worker, args=(w, port + i, str(base), data, data33, rccl), nprocs=w, join=True, start_method="spawn")
    return str(base)


def _load(runs, tag, step, world):
    return [np.load(os.path.join(runs, "%s_s%d_w%d_r%d.npz" % (tag, step, world, g))) for g in range(max(world, 1))]


def _one(runs, tag, step):
    return np.load(os.path.join(runs, "%s_s%d_w1_r0.npz" % (tag, step)))


def _equal_one_process(ranks, one, steps, exact_loss=False):
    """Every rank's gathered tables, relation slots and rng streams equal the one-process run's bit for bit, the union of the
    ranks' entity slot rows too; the losses of its last `steps` steps (both runs end at the same step) to 1e-5 relative."""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for r in ranks:
        assert np.array_equal(r["states"], one["states"])
        for k in ("ent_embeddings", "rel_embeddings"):
            assert r[k].shape == one[k].shape and np.array_equal(bits(r[k]), bits(one[k])), k
        got, want = r["losses"], one["losses"][-steps:]
        assert len(got) == steps and len(want) == steps and (want > 0).all()
        assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), (got, want)
        if exact_loss:
            assert np.array_equal(got, want)
        for k in one.files:
            if k.endswith("_rel") and k[0] in "mva":
                assert np.array_equal(bits(r[k]), bits(one[k])), k
    for k in [k for k in one.files if k.endswith("_ent") and k[0] in "mva"]:      # the slot rows: the ranks' shards side by side
        assert [int(r["lo"]) for r in ranks] == sorted(int(r["lo"]) for r in ranks)
        union = np.concatenate([r[k] for r in ranks])
        assert union.shape == one[k].shape and np.array_equal(bits(union), bits(one[k])), k


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("world", [2, 3, 4])
def test_ranks_equal_the_one_process_shared_run(runs, world, opt):
    ranks, one = _load(runs, "main_" + opt, 3, world), _one(runs, "main_" + opt, 3)
    assert int(one["batch"]) % P != 0
    assert any(int(r["first_pos"]) % P for r in ranks)      # a slice bound inside a chunk
    _equal_one_process(ranks, one, 3)
    if opt != "SGD":
        assert any(k.endswith("_ent") for k in one.files)


@pytest.mark.parametrize("opt", ["SGD", "LazyAdam"])
def test_an_empty_shard(runs, opt):
    ranks = _load(runs, "e33_" + opt, 3, 8)
    assert int(ranks[7]["lo"]) == int(ranks[7]["hi"]) == 33
    _equal_one_process(ranks, _one(runs, "e33_" + opt, 3), 3)


def test_empty_slices(runs):
    ranks = _load(runs, "five", 3, 4)
    assert int(ranks[0]["batch"]) == 5
    n_pos = [int(r["traffic"][0, 0]) for r in ranks]
    assert sum(n_pos) == 5 and 0 in n_pos
    _equal_one_process(ranks, _one(runs, "five", 3), 3)


@pytest.mark.parametrize("opt", OPTS)
def test_one_rank_rccl_group_equals_the_shared_step(runs, opt):
    r = np.load(os.path.join(runs, "main_%s_s3_w0_r0.npz" % opt))
    _equal_one_process([r], _one(runs, "main_" + opt, 3), 3, exact_loss=True)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_counted_traffic(runs, world):
    """Per rank and step: rows requested = 2 n_pos + n_chunks N less the ids outside the table, entity records sent = the
    entity-side keys >= 0; over the ranks, what is requested is served and what is sent is received."""
    ranks = _load(runs, "main_SGD", 3, world)
    B = int(ranks[0]["batch"])
    per_step = np.stack([r["traffic"] for r in ranks])      # [rank, step, 8]
    assert per_step.shape == (world, 3, 8)
    n_pos, n_chunks, outside, req, served, sent, received, keyed = np.moveaxis(per_step, 2, 0)
    assert (n_pos.sum(0) == B).all()
    assert np.array_equal(req, 2 * n_pos + n_chunks * N - outside)
    assert np.array_equal(sent, keyed) and (sent > 0).all()
    assert np.array_equal(req.sum(0), served.sum(0)) and np.array_equal(sent.sum(0), received.sum(0))
    # a chunk cut by a slice bound is requested by both ranks: at most one more chunk per rank than one process has
    assert (n_chunks.sum(0) <= -(-B // P) + world - 1).all()
    print("world %d: %.3f rows requested and %.3f records sent per positive (unshared: %d and at most %d)"
          % (world, req.sum() / n_pos.sum(), sent.sum() / n_pos.sum(), 2 + N, 2 + N))
    assert req.sum() < 0.6 * n_pos.sum() * (2 + N)


@pytest.mark.parametrize("world", [4, 1])
def test_a_checkpoint_resumes_at_another_rank_count(runs, world):
    """Two steps on 2 ranks, saved; resumed on 4 ranks and in one process for two more: four uninterrupted one-process steps."""
    files = sorted(os.listdir(os.path.join(runs, "ckpt")))
    assert {"model.ckpt-2.npz", "model.ckpt-2.shard0of2.npz", "model.ckpt-2.shard1of2.npz"} <= set(files)
    z = np.load(os.path.join(runs, "ckpt", "model.ckpt-2.npz"))
    assert [int(x) for x in z["shared_negatives"]] == [P, SEED] and "ent_embeddings" not in z.files
    _equal_one_process(_load(runs, "resumed", 4, world), _one(runs, "main_" + CKPT_OPT, 4), 2)


def test_refusals(runs):
    for g in range(2):
        said = json.load(open(os.path.join(runs, "refusals_w2_r%d.json" % g)))
        assert "shared negatives" in said["resume_chunk"] and "(4, %d)" % SEED in said["resume_chunk"]
        assert "shared negatives" in said["resume_seed"] and str(SEED + 1) in said["resume_seed"]
        assert "multiple of 4" in said["width"] and "50" in said["width"]
        assert "type-constrained" in said["typed"]
        assert "shared negatives" in said["persistent"] and "persistent" in said["persistent"]
