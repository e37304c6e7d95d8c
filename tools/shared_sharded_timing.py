#!/usr/bin/env python3
"""What shared negatives change in the step on a ROW-SHARDED entity table (train_paths.shared_sharded_step against
train_paths.sharded_step), on one MI355X.

No multi-GPU node exists here, so this measures the step's own machinery on a ONE-rank RCCL group (`force_data_parallel`, backend
"nccl"): request list, counting sort by owner, the owner's row gather, remap, emit over the fetched rows, record packing, reduce
and apply -- every stage and every collective of the N-rank step, with nothing on a wire.  What N ranks add is the wire itself; the
rows and records that would cross it are COUNTED here (Config.last_exchange_sizes), exact integers that do not depend on the
rank count beyond the chunks a slice bound cuts.

Shape: the 5 M x 200 table (4 GB) of DESIGN 4.1.2, 8 M uniform random triples, B = 131 147, n = 25, TransE with SGD, Bernoulli sides.
Variants: the unshared sharded step from --baseline-root (the commit this one is compared with; default: this tree), the unshared
step of this tree, and the shared step at chunks of P = 16 and 64 positives.

Protocol of tools/shared_negatives_timing.py: the engine is one per process, so every measurement is a child process of this
driver with a time limit of its own; the driver alternates the variants over --rounds rounds, stops at the first child that
fails, and appends one JSON line per child to --out (default profiles/shared_sharded.jsonl) and a summary line (medians and
ranges) at the end.  Step time: host clock around --steps steps that end in a device synchronise, after --warmup steps.

usage: shared_sharded_timing.py [--rounds 3] [--steps 50] [--warmup 5] [--limit 300] [--out FILE] [--baseline-root DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(E=5_000_000, R=1000, D=200, triples=8_000_000, nbatches=61, n=25)
CHUNKS = (16, 64)


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(a.port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    import openkeonspark_amd as ok
    s = SHAPE
    rng = np.random.default_rng(5)
    h = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
    t = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
    r = rng.integers(0, s["R"], s["triples"], dtype=np.int64)
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(s["D"]); con.set_ent_neg_rate(s["n"]); con.set_rel_neg_rate(0)
    con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method("SGD"); con.set_nbatches(s["nbatches"])
    con.sparse_rows = True
    con.prefetch_sampling = False
    if a.chunk:
        con.set_shared_negatives(a.chunk, seed=1)
    con.init_from_arrays(s["E"], s["R"], h, t, r)
    del h, t, r
    con.set_model_and_session(ok.TransE)
    con.force_data_parallel = True
    con.init_distributed()
    assert con.sparse_rows and con._dp and con._sharded("ent_embeddings")
    for _ in range(a.warmup):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = con.train_step(sync=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B = con.batch_size
    res = dict(tool="shared_sharded_timing", chunk=a.chunk, root="this tree" if os.path.abspath(a.root) == ROOT else "baseline",
               entities=s["E"], dim=s["D"], batch=B, negatives=s["n"], steps=a.steps, step_us=round(dt / a.steps * 1e6, 2),
               loss=float(loss.item()))
    sizes = con.last_exchange_sizes() if hasattr(con, "last_exchange_sizes") else None      # (the last step's; the baseline has no accessor)
    if sizes:
        res.update(rows_requested=sizes["rows_requested"], records_sent=sizes["records_sent"],
                   rows_requested_per_positive=round(sizes["rows_requested"] / B, 4),
                   records_sent_per_positive=round(sizes["records_sent"] / B, 4))
    print("RESULT " + json.dumps(res), flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_sharded.jsonl"))
    ap.add_argument("--baseline-root", default=ROOT)
    ap.add_argument("--port", type=int, default=36700)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    variants = [("unshared_baseline", 0, a.baseline_root), ("unshared", 0, ROOT)] + [("P%d" % c, c, ROOT) for c in CHUNKS]
    seen, port = {}, a.port
    for rnd in range(a.rounds):
        for name, chunk, root in variants:
            port += 1
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--chunk", str(chunk), "--root", root, "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--port", str(port)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print("child %s ran into its limit of %d s: stopping" % (name, a.limit), file=sys.stderr)
                return 2
            lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                print("child %s failed (exit %d): stopping\n%s" % (name, p.returncode, p.stderr[-2000:]), file=sys.stderr)
                return p.returncode or 1
            res = json.loads(lines[-1][7:])
            res["round"], res["variant"] = rnd, name
            print(json.dumps(res), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(res) + "\n")
            seen.setdefault(name, []).append(res)
    med = lambda rs, k: statistics.median(x[k] for x in rs)
    rng_ = lambda rs, k: [min(x[k] for x in rs), max(x[k] for x in rs)]
    base = seen["unshared_baseline"]
    summary = dict(tool="shared_sharded_timing", summary="large, one-rank RCCL group", rounds=a.rounds, batch=base[0]["batch"],
                   negatives=base[0]["negatives"], unshared_from=base[0]["root"])
    for name, _, _ in variants:
        rs = seen[name]
        summary[name] = dict(step_us=med(rs, "step_us"), step_us_range=rng_(rs, "step_us"),
                             step_ratio_to_unshared_baseline=round(med(rs, "step_us") / med(base, "step_us"), 3))
        for k in ("rows_requested_per_positive", "records_sent_per_positive"):
            if k in rs[0]:
                summary[name][k] = rs[0][k]
    print(json.dumps(summary), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(summary) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
