"""Digests of five sampled training steps on every step path, for comparing two commits bit for bit.

    python tools/step_digests.py OUT.json

For each cell (a model, an optimizer, a width, a world size and the switches that pick a step path) it trains 5 steps on a
synthetic graph (E = 200, R = 7, batch 64) and records the SHA-256 of every table and every optimizer slot and the five losses
as hex floats.  Only Config's public methods and documented attributes are used, so the same file runs at any commit.  Run it
twice at one commit to learn which cells are reproducible there (the fp32-atomic paths are not); those must then agree between
two commits that claim the same arithmetic.  One-rank cells share a process; two-rank cells share one gloo group of two
processes on the one GPU; the `force_data_parallel` cells run in a one-rank RCCL group."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, R, BATCH, NBATCHES, STEPS = 200, 7, 64, 20, 5
ROWS_OPTS = ("SGD", "LazyAdam", "Adagrad")


def cells():
    """-> (one-rank cells, one-rank RCCL-group cells, two-rank cells); a cell is a dict of the worker's keyword arguments."""
    one, forced, two = [], [], []

    def cell(dest, name, model, opt, dim=8, **attrs):
        dest.append(dict(name=name, model=model, opt=opt, dim=dim, attrs=attrs))

    for opt in ROWS_OPTS:
        for model in ("TransE", "TransH", "TransD"):      # in-place rows from float records
            attrs = dict(sparse_rows=True, **(dict(use_counts=False) if model == "TransE" else {}))
            cell(one, "inplace/%s/%s/w1" % (model, opt), model, opt, **attrs)
            cell(two, "inplace/%s/%s/w2" % (model, opt), model, opt, **attrs)
        sparse = dict(sparse_rows=True, counts_min_records=0)
        cell(one, "sparse/%s/fused" % opt, "TransE", opt, sparse_fused=True, **sparse)
        cell(one, "sparse/%s/unfused" % opt, "TransE", opt, sparse_fused=False, **sparse)
        cell(one, "sparse/%s/d6" % opt, "TransE", opt, dim=6, **sparse)
        cell(two, "sharded/%s/relneg0" % opt, "TransE", opt, **sparse)
        cell(two, "sharded/%s/relneg1" % opt, "TransE", opt, negative_rel=1, **sparse)
        cell(forced, "sharded/%s/forced_w1" % opt, "TransE", opt, force_data_parallel=True, **sparse)
    for opt in ("SGD", "Adam"):
        for fused in (True, False):
            cell(one, "counts/%s/fused_counts=%s" % (opt, fused), "TransE", opt, counts_min_records=0, fused_counts=fused)
        for pieces in (1, 2):
            cell(two, "counts/%s/w2/pieces%d" % (opt, pieces), "TransE", opt, counts_min_records=0, dp_pieces=pieces)
        cell(one, "dense/TransH/%s/w1" % opt, "TransH", opt)
        cell(two, "dense/TransH/%s/w2" % opt, "TransH", opt)
        cell(one, "persistent/TransE/%s" % opt, "TransE", opt, persistent=True)
    cell(one, "dense/TransR/SGD", "TransR", "SGD")
    cell(one, "dense/TransR/Adagrad", "TransR", "Adagrad")
    return one, forced, two


def graph():
    sys.path.insert(0, ROOT)
    from openkeonspark_amd.synthetic import generate_triples
    h, t, r = generate_triples(E, R, 4 * BATCH * NBATCHES, seed=11, dup_frac=0.0)
    _, first = np.unique(np.stack([h, t, r]), axis=1, return_index=True)
    keep = np.sort(first)[:BATCH * NBATCHES]
    assert len(keep) == BATCH * NBATCHES
    return h[keep], t[keep], r[keep]


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def run_cell(pkg, c, triples, distributed):
    import torch
    attrs = dict(c["attrs"])
    con = pkg.Config()
    con.set_work_threads(8); con.set_bern(0); con.set_dimension(c["dim"]); con.set_nbatches(NBATCHES)
    con.set_ent_neg_rate(2); con.set_rel_neg_rate(attrs.pop("negative_rel", 0)); con.set_alpha(0.05); con.set_opt_method(c["opt"])
    persistent = attrs.pop("persistent", False)
    for k, v in attrs.items():
        setattr(con, k, v)
    con.init_from_arrays(E, R, *triples)
    assert con.batch_size == BATCH
    con.set_model_and_session(getattr(pkg, c["model"]))
    if distributed:
        con.init_distributed()
    if persistent:
        losses = [float(x) for x in con.train_steps(STEPS, persistent=True)]
    else:
        losses = [con.train_step() for _ in range(STEPS)]
    con.sync_optimizer_state()
    torch.cuda.synchronize()
    out = dict(losses=[float(x).hex() for x in losses], global_step=int(con.global_step))
    for name, value in con.get_parameters().items():      # (collective on a sharded table: every rank gets the whole table)
        out[name] = hashlib.sha256(np.ascontiguousarray(value).tobytes()).hexdigest()
    for slot in ("_adam_m", "_adam_v", "_adagrad_acc"):      # this rank's slots (shard-sized where the entity table is sharded)
        if (slot == "_adagrad_acc" and con._adagrad) or (slot != "_adagrad_acc" and con._has_slots):
            for name, t in zip(con.trainModel.table_names, getattr(con, slot)):
                out["%s/%s" % (slot, name)] = sha(t)
    out["path"] = "use_counts=%d sparse_rows=%d sparse_inplace=%d" % (con.use_counts, con.sparse_rows, con.sparse_inplace)
    return out


def worker(rank, world, port, backend, todo, out_path):
    sys.path.insert(0, ROOT)
    import torch
    import openkeonspark_amd as pkg
    if backend:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        torch.cuda.set_device(0)
        dist.init_process_group(backend, rank=rank, world_size=world)
    triples = graph()
    res = {}
    for c in todo:
        res["%s#r%d" % (c["name"], rank)] = run_cell(pkg, c, triples, bool(backend))
        print("done", c["name"], "rank", rank, flush=True)
    with open("%s.part%d_%s" % (out_path, rank, backend or "one"), "w") as f:
        json.dump(res, f)
    if backend:
        dist.barrier()
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    out_path = os.path.abspath(sys.argv[1])
    one, forced, two = cells()
    port = 29300 + os.getpid() % 500
    mp.start_processes(worker, args=(1, port, None, one, out_path), nprocs=1, join=True, start_method="spawn")
    mp.start_processes(worker, args=(1, port + 1, "nccl", forced, out_path), nprocs=1, join=True, start_method="spawn")
    mp.start_processes(worker, args=(2, port + 2, "gloo", two, out_path), nprocs=2, join=True, start_method="spawn")
    res = {}
    for part in ("0_one", "0_nccl", "0_gloo", "1_gloo"):
        with open("%s.part%s" % (out_path, part)) as f:
            res.update(json.load(f))
        os.remove("%s.part%s" % (out_path, part))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("%d cells, %d digests" % (len(one) + len(forced) + len(two), len(res)))


if __name__ == "__main__":
    main()
