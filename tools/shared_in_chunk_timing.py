#!/usr/bin/env python3
"""What IN-CHUNK candidates of relation-grouped shared negatives (Config.set_shared_negatives(..., by_relation=True, in_chunk=K);
NON-PARITY, opt-in) cost against drawn ones, on one MI355X.  In the manner of tools/shared_grouped_timing.py.

Two shapes, SGD on sparse rows, Bernoulli sides, typed candidates, P = 64:
  headline  the FB15k-237-shaped typed graph synthetic.FB15K237_TYPED (E = 14 541, R = 237, type_constrain.txt), D = 200,
            B = 34 014; TransE and TransH
  large     the 5 M x 200 table (4 GB): 8 M uniform triples over R = 1000 relations, B = 131 147, lists derived from the triples;
            TransE only
Per shape and model, five variants of the grouped step at equal B and P:
  parent    (N, K) = (25, 0) from the built checkout in --baseline-root: the baseline
  n25_k0    the same step from this tree (must lie within the parent's own round-to-round range)
  n50_k0 and n25_k25   equal pairs: what an in-chunk column costs against a drawn one
  n13_k12   against n25_k0
and per variant of this tree, counted exactly on the last step: n_chunks, the -1 columns, the masked pairs of the drawn and of the
in-chunk columns; with --stages 1 the draw stage alone (device events around 20 launches on the last batch, after 3): the grouped
draw kernel at N + K drawn columns against the mixed kernel at (N, K).

The engine is one per process, so every measurement is a child process of this driver with a time limit of its own; the driver
alternates the variants over --rounds rounds, stops at the first child that fails, and appends one JSON line per child and one
summary line per (shape, model) -- medians and ranges -- to --out (default profiles/shared_in_chunk.jsonl).
Step time: host clock around --steps steps that end in a device synchronise, after --warmup steps.

--metrics STEPS: also train synthetic.SMALL_TYPED (D = 64, B = 1000, P = 16, Adagrad, grouped untyped) for STEPS steps at (N, K) =
(25, 0), (13, 12) and (25, 25) and print each run's TYPED FILTERED Hits@10 and MRR from link_prediction over the test split.  A
one-seed report on a synthetic graph, not a gate.

usage: shared_in_chunk_timing.py [--shapes headline,large] [--models TransE,TransH] [--rounds 3] [--steps 60] [--warmup 10]
                                 [--stages 1] [--limit 300] [--out FILE] [--baseline-root DIR] [--data DIR] [--metrics STEPS]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"headline": dict(D=200, nbatches=8), "large": dict(E=5_000_000, R=1000, D=200, triples=8_000_000, nbatches=61)}
VARIANTS = {"parent": (25, 0), "n25_k0": (25, 0), "n50_k0": (50, 0), "n25_k25": (25, 25), "n13_k12": (13, 12)}
METRIC_RUNS = {"n25_k0": (25, 0), "n13_k12": (13, 12), "n25_k25": (25, 25)}
CHUNK = 64


def configure(ok, s, model, N, K, chunk, typed, data, keyword):
    import numpy as np
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(s["D"]); con.set_ent_neg_rate(N); con.set_rel_neg_rate(0)
    con.set_alpha(s.get("alpha", 0.01)); con.set_margin(1.0); con.set_opt_method(s.get("opt", "SGD")); con.set_nbatches(s["nbatches"])
    con.sparse_rows = True
    if keyword:
        con.set_shared_negatives(chunk, seed=1, by_relation=True, in_chunk=K)
    else:
        con.set_shared_negatives(chunk, seed=1, by_relation=True)      # (the parent's signature)
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
    con.set_model_and_session(getattr(ok, model))
    return con


def child(a):
    sys.path.insert(0, a.root)
    import torch
    import openkeonspark_amd as ok
    from openkeonspark_amd import _lib
    s = SHAPES[a.shape]
    N, K = VARIANTS[a.variant]
    con = configure(ok, s, a.model, N, K, CHUNK, True, a.data if a.shape == "headline" else None, a.variant != "parent")
    for _ in range(a.warmup):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = con.train_step(sync=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B = con.batch_size
    res = dict(tool="shared_in_chunk_timing", shape=a.shape, model=a.model, chunk=CHUNK, variant=a.variant, drawn=N, in_chunk=K,
               entities=con.entTotal, relations=con.relTotal, dim=s["D"], batch=B, steps=a.steps, step_us=round(dt / a.steps * 1e6, 2),
               loss=float(loss.item()))
    cand, pair, perm, chunks = con.shared_negatives_of(con.global_step - 1)
    masked = (pair & 2) != 0
    res.update(n_chunks=len(chunks), chunks_by_position=-(-B // CHUNK), minus_one_columns=int((cand < 0).sum()),
               masked_drawn=int(masked[:, :N].sum()), pairs_drawn=B * N, masked_in_chunk=int(masked[:, N:].sum()), pairs_in_chunk=B * K)
    if a.stages and a.variant != "parent":
        L, st, buf = con.lib, con._stream(), con._sparse_buf
        h2, t2, r2 = (buf["sorted"][i].data_ptr() for i in range(3))
        tab, cap = buf["chunks"].data_ptr(), buf["chunks"].shape[0]
        cand2, pair2 = torch.empty_like(buf["cand"]), torch.empty_like(buf["pair"])
        step = con.global_step - 1

        def timed(call):
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                call()
            e1.record()
            torch.cuda.synchronize()
            return round(e0.elapsed_time(e1) / 20 * 1e3, 2)
        res["draw_old_us"] = timed(lambda: _lib.check(L.kge_shared_negatives_draw_grouped(
            h2, t2, r2, B, tab, cap, N + K, 1, 1, step, cand2.data_ptr(), pair2.data_ptr(), st), L))
        res["draw_mixed_us"] = timed(lambda: _lib.check(L.kge_shared_negatives_draw_grouped_mixed(
            h2, t2, r2, B, tab, cap, N, K, 1, 1, step, cand2.data_ptr(), pair2.data_ptr(), st), L))
        assert torch.equal(cand2, buf["cand"]) and torch.equal(pair2, buf["pair"])      # (the mixed entry point repeats the step's lists)
    print("RESULT " + json.dumps(res), flush=True)


def metrics_child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    import openkeonspark_amd as ok
    s = dict(D=64, nbatches=20, opt="Adagrad", alpha=0.1, test=True)
    N, K = METRIC_RUNS[a.variant]
    con = configure(ok, s, "TransE", N, K, 16, False, a.data, True)
    for _ in range(a.steps):
        loss = con.train_step(sync=False)
    torch.cuda.synchronize()
    out, _ = con.link_prediction()
    rank = out[:, :, 3].astype(np.float64) + 1.0          # filtered + typed: candidates scoring strictly below the true triple, plus one
    res = dict(tool="shared_in_chunk_timing", metrics=a.variant, graph="SMALL_TYPED", dim=s["D"], batch=con.batch_size, drawn=N, in_chunk=K,
               chunk=16, optimizer=s["opt"], steps=a.steps, loss=float(loss.item()), test_triples=int(out.shape[0]),
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
    ap.add_argument("--models", default="TransE,TransH")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stages", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_in_chunk.jsonl"))
    ap.add_argument("--baseline-root", default=ROOT)
    ap.add_argument("--data", default=None, help="where the synthetic datasets are written (default: a temporary directory)")
    ap.add_argument("--metrics", type=int, default=0, help="steps of the SMALL_TYPED metric report (0 = none)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--metrics-child", action="store_true")
    ap.add_argument("--shape", default="headline")
    ap.add_argument("--model", default="TransE")
    ap.add_argument("--variant", default="n25_k0")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.metrics_child:
        return metrics_child(a)
    sys.path.insert(0, ROOT)
    from openkeonspark_amd import synthetic
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    base = a.data or tempfile.mkdtemp(prefix="shared_in_chunk_")

    def log(res):
        print(json.dumps(res), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")

    med = lambda rs, k: statistics.median(x[k] for x in rs)
    rng_ = lambda rs, k: [min(x[k] for x in rs), max(x[k] for x in rs)]
    for shape in [x for x in a.shapes.split(",") if x]:
        data = synthetic.make_typed_dataset(os.path.join(base, "fb15k237_typed"), synthetic.FB15K237_TYPED) if shape == "headline" else ""
        for model in [m for m in a.models.split(",") if m and (shape == "headline" or m == "TransE")]:
            seen = {}
            for rnd in range(a.rounds):
                for variant in VARIANTS:
                    root = a.baseline_root if variant == "parent" else ROOT
                    res = run_child(a, ["--child", "--shape", shape, "--model", model, "--variant", variant, "--root", root, "--steps",
                                        str(a.steps), "--warmup", str(a.warmup), "--stages", str(a.stages), "--data", data])
                    if res is None:
                        return 1
                    res["round"] = rnd
                    log(res)
                    seen.setdefault(variant, []).append(res)
            parent = seen["parent"]
            summary = dict(tool="shared_in_chunk_timing", summary=shape, model=model, chunk=CHUNK, rounds=a.rounds, batch=parent[0]["batch"],
                           parent_step_us=med(parent, "step_us"), parent_step_us_range=rng_(parent, "step_us"))
            for variant in list(VARIANTS)[1:]:
                rs = seen[variant]
                d = dict(step_us=med(rs, "step_us"), step_us_range=rng_(rs, "step_us"), n_chunks=rs[-1]["n_chunks"],
                         minus_one_columns=rs[-1]["minus_one_columns"],
                         masked_share_drawn=round(rs[-1]["masked_drawn"] / rs[-1]["pairs_drawn"], 6),
                         masked_share_in_chunk=round(rs[-1]["masked_in_chunk"] / max(rs[-1]["pairs_in_chunk"], 1), 6))
                if a.stages:
                    d.update(draw_old_us=med(rs, "draw_old_us"), draw_mixed_us=med(rs, "draw_mixed_us"))
                summary[variant] = d
            lo, hi = summary["parent_step_us_range"]
            summary["n25_k0_within_parent_range"] = bool(lo <= summary["n25_k0"]["step_us"] <= hi)
            summary["in_chunk_to_drawn_at_50"] = round(summary["n25_k25"]["step_us"] / summary["n50_k0"]["step_us"], 4)
            summary["in_chunk_to_drawn_at_25"] = round(summary["n13_k12"]["step_us"] / summary["n25_k0"]["step_us"], 4)
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
