#!/usr/bin/env python3
"""What shared negatives on RELATION-GROUPED chunks with typed candidates (Config.set_shared_negatives(..., by_relation=True) with
set_type_constrained_sampling; NON-PARITY, opt-in) cost against the plain shared step, on one MI355X.

Two shapes, TransE with SGD on sparse rows, Bernoulli sides, N = 25:
  headline  the FB15k-237-shaped typed graph synthetic.FB15K237_TYPED (E = 14 541, R = 237, type_constrain.txt), D = 200,
            B = 34 014, chunks of P = 16 and 64
  large     the 5 M x 200 table (4 GB): 8 M uniform triples over R = 1000 relations, B = 131 147, P = 64; its type lists are
            derived from the triples (each relation's distinct heads and tails)
Per shape and P, four variants of the step at equal B, P and N:
  parent          the plain shared step (untyped, chunks by position) of the built checkout in --baseline-root: the baseline
  shared          the same step from this tree (must lie within the parent's own round-to-round range)
  grouped         chunks by relation, untyped candidates
  grouped_typed   chunks by relation, candidates from the relations' type lists
and per grouped case: the ordering stage alone (device events around 20 launches of kge_shared_order_by_relation on the last
batch, after 3), n_chunks / ceil(B / P) counted on the last step, the share of masked pairs and the share of fallback candidates
(candidates of used chunks drawn from all entities: every one when untyped, those of a relation without a list on the
candidate's side when typed).

The engine is one per process, so every measurement is a child process of this driver with a time limit of its own; the driver
alternates the variants over --rounds rounds, stops at the first child that fails, and appends one JSON line per child and one
summary line per (shape, P) -- medians and ranges -- to --out (default profiles/shared_grouped.jsonl).
Step time: host clock around --steps steps that end in a device synchronise, after --warmup steps.

--metrics STEPS: also train synthetic.SMALL_TYPED (D = 64, N = 25, P = 16, Adagrad) for STEPS steps in four ways -- unshared
untyped, unshared typed, shared untyped, shared grouped typed -- and print each run's TYPED FILTERED Hits@10 and MRR from
link_prediction over the test split.  A report on a synthetic graph, not a gate.

usage: shared_grouped_timing.py [--shapes headline,large] [--rounds 3] [--steps 100] [--warmup 10] [--limit 300] [--out FILE]
                                [--baseline-root DIR] [--data DIR] [--metrics STEPS]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"headline": dict(D=200, nbatches=8, n=25, chunks=(16, 64)),
          "large": dict(E=5_000_000, R=1000, D=200, triples=8_000_000, nbatches=61, n=25, chunks=(64,))}
VARIANTS = ("parent", "shared", "grouped", "grouped_typed")
METRIC_RUNS = ("unshared", "unshared_typed", "shared", "shared_grouped_typed")


def configure(ok, a, s, shared, by_relation, typed, data):
    import numpy as np
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(s["D"]); con.set_ent_neg_rate(s["n"]); con.set_rel_neg_rate(0)
    con.set_alpha(s.get("alpha", 0.01)); con.set_margin(1.0); con.set_opt_method(s.get("opt", "SGD")); con.set_nbatches(s["nbatches"])
    con.sparse_rows = True
    if shared:
        if by_relation:
            con.set_shared_negatives(a.chunk, seed=1, by_relation=True)
        else:
            con.set_shared_negatives(a.chunk, seed=1)      # (the parent's signature)
    if data:      # a dataset directory with type_constrain.txt
        con.set_in_path(data)
        if s.get("test"):
            con.set_test_link_prediction(True)
        con.set_type_constrained_sampling(typed)
        con.init()
    else:
        rng = np.random.default_rng(5)
        h = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
        t = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
        r = rng.integers(0, s["R"], s["triples"], dtype=np.int64)
        con.init_from_arrays(s["E"], s["R"], h, t, r)
        if typed:
            empty = (np.zeros(0, np.int64),) * 3
            con.init_evaluation_from_arrays(empty, empty, derive_types=True)
            con.set_type_constrained_sampling(True)
    con.set_model_and_session(ok.TransE)
    return con


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    import openkeonspark_amd as ok
    from openkeonspark_amd import _lib
    s = SHAPES[a.shape]
    grouped, typed = a.variant.startswith("grouped"), a.variant == "grouped_typed"
    con = configure(ok, a, s, True, grouped, typed, a.data if a.shape == "headline" else None)
    assert con.sparse_rows
    for _ in range(a.warmup):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = con.train_step(sync=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B, n, P = con.batch_size, s["n"], a.chunk
    res = dict(tool="shared_grouped_timing", shape=a.shape, chunk=P, variant=a.variant, entities=con.entTotal, relations=con.relTotal,
               dim=s["D"], batch=B, negatives=n, steps=a.steps, step_us=round(dt / a.steps * 1e6, 2), loss=float(loss.item()))
    buf = con._sparse_buf
    if grouped:
        L, st = con.lib, con._stream()
        dev = buf["shared_batch"]
        scratch = {k: torch.empty_like(buf[k]) for k in ("perm", "sorted", "chunks", "n_chunks")}

        def order():
            _lib.check(L.kge_shared_order_by_relation(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), B, P, scratch["perm"].data_ptr(),
                                                      scratch["sorted"][0].data_ptr(), scratch["sorted"][1].data_ptr(),
                                                      scratch["sorted"][2].data_ptr(), scratch["chunks"].data_ptr(),
                                                      scratch["n_chunks"].data_ptr(), st), L)
        for _ in range(3):
            order()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            order()
        e1.record()
        torch.cuda.synchronize()
        res["order_us"] = round(e0.elapsed_time(e1) / 20 * 1e3, 2)
        cand, pair, perm, chunks = con.shared_negatives_of(con.global_step - 1)
        assert np.array_equal(scratch["chunks"][:len(chunks)].cpu().numpy(), chunks)
        n_chunks = len(chunks)
        res["n_chunks"], res["chunks_by_position"] = n_chunks, -(-B // P)
        res["chunk_ratio"] = round(n_chunks / -(-B // P), 4)
        res["cap"] = int(buf["chunks"].shape[0])
        res["masked_share"] = round(float(((pair & 2) != 0).mean()), 6)
        if typed:
            head_off, _, tail_off, _ = con.type_constraints()
            rel = buf["sorted"][2][:B].cpu().numpy()[chunks[:, 0]]                     # the relation of every used chunk
            new_head = (pair[chunks[:, 0]] & 1) == 1                                  # [n_chunks, N]: the side of every candidate
            ok_rel = (rel >= 0) & (rel < con.relTotal)
            rel0 = np.where(ok_rel, rel, 0)
            listed = np.where(new_head, np.diff(head_off)[rel0][:, None], np.diff(tail_off)[rel0][:, None]) > 0
            res["fallback_share"] = round(float(1.0 - (listed & ok_rel[:, None]).mean()), 6)
        else:
            res["fallback_share"] = 1.0
    else:
        res["masked_share"] = round(float(((con.shared_negatives_of(con.global_step - 1)[1] & 2) != 0).mean()), 6)
    print("RESULT " + json.dumps(res), flush=True)


def metrics_child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    import openkeonspark_amd as ok
    s = dict(D=64, nbatches=20, n=25, opt="Adagrad", alpha=0.1, test=True)
    a.chunk = 16
    run = a.variant
    con = configure(ok, a, s, run.startswith("shared"), run == "shared_grouped_typed", run.endswith("typed"), a.data)
    for _ in range(a.steps):
        loss = con.train_step(sync=False)
    torch.cuda.synchronize()
    out, _ = con.link_prediction()
    rank = out[:, :, 3].astype(np.float64) + 1.0          # filtered + typed: candidates scoring strictly below the true triple, plus one
    res = dict(tool="shared_grouped_timing", metrics=run, graph="SMALL_TYPED", dim=s["D"], batch=con.batch_size, negatives=s["n"], chunk=a.chunk,
               optimizer=s["opt"], steps=a.steps, loss=float(loss.item()), test_triples=int(out.shape[0]),
               typed_filtered_hits10=round(float((rank <= 10).mean()), 4), typed_filtered_mrr=round(float((1.0 / rank).mean()), 4))
    print("RESULT " + json.dumps(res), flush=True)


def run_child(a, args):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        print("child %s ran into its limit of %d s: stopping" % (args, a.limit), file=sys.stderr)
        return None
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        print("child %s failed (exit %d): stopping\n%s" % (args, p.returncode, p.stderr[-2000:]), file=sys.stderr)
        return None
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,large")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_grouped.jsonl"))
    ap.add_argument("--baseline-root", default=ROOT)
    ap.add_argument("--data", default=None, help="where the synthetic datasets are written (default: a temporary directory)")
    ap.add_argument("--metrics", type=int, default=0, help="steps of the SMALL_TYPED metric report (0 = none)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--metrics-child", action="store_true")
    ap.add_argument("--shape", default="headline")
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--variant", default="shared")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.metrics_child:
        return metrics_child(a)
    sys.path.insert(0, ROOT)
    from openkeonspark_amd import synthetic
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    base = a.data or tempfile.mkdtemp(prefix="shared_grouped_")

    def log(res):
        print(json.dumps(res), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")

    med = lambda rs, k: statistics.median(x[k] for x in rs)
    rng_ = lambda rs, k: [min(x[k] for x in rs), max(x[k] for x in rs)]
    for shape in [x for x in a.shapes.split(",") if x]:
        data = synthetic.make_typed_dataset(os.path.join(base, "fb15k237_typed"), synthetic.FB15K237_TYPED) if shape == "headline" else ""
        for chunk in SHAPES[shape]["chunks"]:
            seen = {}
            for rnd in range(a.rounds):
                for variant in VARIANTS:
                    root = a.baseline_root if variant == "parent" else ROOT
                    res = run_child(a, ["--child", "--shape", shape, "--chunk", str(chunk), "--variant", variant, "--root", root, "--steps",
                                        str(a.steps), "--warmup", str(a.warmup), "--data", data])
                    if res is None:
                        return 1
                    res["round"] = rnd
                    log(res)
                    seen.setdefault(variant, []).append(res)
            parent = seen["parent"]
            summary = dict(tool="shared_grouped_timing", summary=shape, chunk=chunk, rounds=a.rounds, batch=parent[0]["batch"],
                           negatives=parent[0]["negatives"], parent_step_us=med(parent, "step_us"), parent_step_us_range=rng_(parent, "step_us"))
            for variant in VARIANTS[1:]:
                rs = seen[variant]
                d = dict(step_us=med(rs, "step_us"), step_us_range=rng_(rs, "step_us"),
                         step_ratio_to_parent=round(med(rs, "step_us") / med(parent, "step_us"), 3), masked_share=med(rs, "masked_share"))
                if variant != "shared":
                    d.update(order_us=med(rs, "order_us"), order_us_range=rng_(rs, "order_us"), n_chunks=rs[-1]["n_chunks"],
                             chunk_ratio=med(rs, "chunk_ratio"), fallback_share=med(rs, "fallback_share"))
                summary[variant] = d
            lo, hi = summary["parent_step_us_range"]
            summary["shared_within_parent_range"] = bool(lo <= summary["shared"]["step_us"] <= hi)
            log(summary)
    if a.metrics:
        data = synthetic.make_typed_dataset(os.path.join(base, "small_typed"), synthetic.SMALL_TYPED)
        for run in METRIC_RUNS:
            res = run_child(a, ["--metrics-child", "--variant", run, "--steps", str(a.metrics), "--data", data])
            if res is None:
                return 1
            log(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
