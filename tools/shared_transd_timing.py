#!/usr/bin/env python3
"""What TransD on shared negatives over RELATION-GROUPED chunks (Config.set_shared_negatives(..., by_relation=True) with the TransD
model; NON-PARITY, opt-in) costs against the unshared TransD touched-rows step, on one MI355X; --model TransH measures TransH the
same way (tools/shared_transh_timing.py is the tool its published figures came from).

Two shapes, SGD on touched rows, Bernoulli sides, N = 25:
  headline  the FB15k-237-shaped typed graph synthetic.FB15K237_TYPED (E = 14 541, R = 237, type_constrain.txt), D = 200,
            B = 34 014, chunks of P = 16 and 64, type-constrained sampling on in every variant
  large     the 5 M x 200 table (TransD: two such tables, 8 GB): 8 M uniform triples over R = 1000 relations, B = 131 147,
            P = 64, untyped
Per shape and P, three variants of the step at equal B and N:
  parent    the unshared touched-rows step (kge_forward_backward_sgd_rows) of the built checkout in --baseline-root: the baseline
  unshared  the same step from this tree (must lie within the parent's own round-to-round range)
  shared    chunks by relation: r^, the relation's transfer (normal) vector and N projected candidates once per chunk
and per shared case: the emit kernel alone (device events around 20 launches on the last step's lists, after 3), n_chunks /
ceil(B / P) counted on the last step, the share of masked pairs and the table rows gathered (derived from the counts).

--stages 1 is a run of its own: per (shape, P) one child per round times the four stages of the shared step ONE BY ONE with device
events -- order (kge_shared_order_by_relation), draw (kge_shared_negatives_draw_grouped), emit, and the float-record apply
(RowsRule.apply_float_records, SGD) -- each over 20 launches after 3 on the last step's inputs, beside the whole step.  The apply
is timed on a copy of the last step's records and keys; it moves the tables, which nothing reads afterwards.

The engine is one per process, so every measurement is a child process of this driver with a time limit of its own; the driver
alternates the variants over --rounds rounds, stops at the first child that fails, and appends one JSON line per child and one
summary line per (shape, P) -- medians and ranges -- to --out (default profiles/shared_transd.jsonl).
Step time: host clock around --steps steps that end in a device synchronise, after --warmup steps.  Convergence is not measured.

usage: shared_transd_timing.py [--model TransD|TransH] [--stages 1] [--shapes headline,large] [--rounds 3] [--steps 100]
                               [--warmup 10] [--limit 300] [--out FILE] [--baseline-root DIR] [--data DIR]"""
import argparse
import ctypes
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
VARIANTS = ("parent", "unshared", "shared")


def configure(ok, a, s, shared, data):
    import numpy as np
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(s["D"]); con.set_ent_neg_rate(s["n"]); con.set_rel_neg_rate(0)
    con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method("SGD"); con.set_nbatches(s["nbatches"])
    con.sparse_rows = True
    if shared:
        con.set_shared_negatives(a.chunk, seed=1, by_relation=True)
    if data:      # a dataset directory with type_constrain.txt
        con.set_in_path(data)
        con.set_type_constrained_sampling(True)
        con.init()
    else:
        rng = np.random.default_rng(5)
        h = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
        t = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
        r = rng.integers(0, s["R"], s["triples"], dtype=np.int64)
        con.init_from_arrays(s["E"], s["R"], h, t, r)
    con.set_model_and_session(getattr(ok, a.model))
    return con


def child(a):
    sys.path.insert(0, a.root)
    import torch
    import openkeonspark_amd as ok
    from openkeonspark_amd import _lib
    s = SHAPES[a.shape]
    shared = a.variant == "shared"
    con = configure(ok, a, s, shared, a.data if a.shape == "headline" else None)
    assert con.sparse_inplace
    for _ in range(a.warmup):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = con.train_step(sync=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B, n, P = con.batch_size, s["n"], a.chunk
    res = dict(tool="shared_transd_timing", model=a.model, shape=a.shape, chunk=P, variant=a.variant, entities=con.entTotal, relations=con.relTotal,
               dim=s["D"], batch=B, negatives=n, steps=a.steps, step_us=round(dt / a.steps * 1e6, 2), loss=float(loss.item()))
    if shared:
        L, st, buf = con.lib, con._stream(), con._sparse_buf
        cand, pair, perm, chunks = con.shared_negatives_of(con.global_step - 1)
        cap = buf["shared_shape"][1]
        rec, dst, out = torch.empty_like(buf["rec"]), torch.empty_like(buf["dst"]), torch.zeros(1, dtype=torch.float32, device=con.device)
        h2, t2, r2 = (buf["sorted"][i].data_ptr() for i in range(3))

        transd = a.model == "TransD"
        emit_fn = L.kge_transd_emit_records_shared_chunks if transd else L.kge_transh_emit_records_shared_chunks
        ew = 2 if transd else 1      # table rows, and records, per entity
        M = 2 * ew * B + cap * (ew * n + 2)

        def emit():
            _lib.check(emit_fn(ctypes.byref(con._desc), con._tab_ptrs, h2, t2, r2, B, B, buf["chunks"].data_ptr(), cap, buf["cand"].data_ptr(),
                               n, buf["pair"].data_ptr(), B * n, B, rec.data_ptr(), dst.data_ptr(), out.data_ptr(), st), L)

        def timed(fn, before=None):
            """us per launch over 20 launches after 3; `before` (untimed) restores what a launch consumes"""
            total = 0.0
            for i in range(23):
                if before:
                    before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    total += e0.elapsed_time(e1)
            return round(total / 20 * 1e3, 2)

        for _ in range(3):
            emit()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            emit()
        e1.record()
        torch.cuda.synchronize()
        res["emit_us"] = round(e0.elapsed_time(e1) / 20 * 1e3, 2)
        if a.stages:
            dev = buf["shared_batch"]
            h, t, r = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
            typed = 1 if con.type_constrained_sampling else 0
            step = con.global_step - 1
            res["order_us"] = timed(lambda: _lib.check(L.kge_shared_order_by_relation(
                h, t, r, B, P, buf["perm"].data_ptr(), h2, t2, r2, buf["chunks"].data_ptr(), buf["n_chunks"].data_ptr(), st), L))
            res["draw_us"] = timed(lambda: _lib.check(L.kge_shared_negatives_draw_grouped(
                h2, t2, r2, B, buf["chunks"].data_ptr(), cap, n, typed, con._shared_seed, step, buf["cand"].data_ptr(), buf["pair"].data_ptr(), st), L))
            res["emit_single_us"] = timed(emit)
            emit()
            dst0 = dst.clone()      # the apply sorts its keys in place: every launch gets a fresh copy

            def restore():
                dst.copy_(dst0)
            res["apply_us"] = timed(lambda: con._rule.apply_float_records(rec, dst, M, B, n), restore)
            res["records"], res["records_keyed"] = int(M), int((dst0 >= 0).sum().item())
            res["stages_sum_us"] = round(res["order_us"] + res["draw_us"] + res["emit_single_us"] + res["apply_us"], 2)
        res["n_chunks"], res["chunks_by_position"], res["cap"] = len(chunks), -(-B // P), int(cap)
        res["chunk_ratio"] = round(len(chunks) / -(-B // P), 4)
        res["masked_share"] = round(float(((pair & 2) != 0).mean()), 6)
        res["rows_gathered"], res["rows_gathered_unshared"] = ew * (2 * B + len(chunks) * n) + 2 * len(chunks), ew * B * (2 + n) + 2 * B
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_transd.jsonl"))
    ap.add_argument("--model", default="TransD", choices=["TransD", "TransH"])
    ap.add_argument("--stages", type=int, default=0, help="1: time the shared step's stages one by one instead of the three variants")
    ap.add_argument("--baseline-root", default=ROOT)
    ap.add_argument("--data", default=None, help="where the synthetic dataset is written (default: a temporary directory)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default="headline")
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--variant", default="shared")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, ROOT)
    from openkeonspark_amd import synthetic
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    base = a.data or tempfile.mkdtemp(prefix="shared_transd_")

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
                for variant in (("shared",) if a.stages else VARIANTS):
                    root = a.baseline_root if variant == "parent" else ROOT
                    res = run_child(a, ["--child", "--shape", shape, "--chunk", str(chunk), "--variant", variant, "--root", root, "--steps",
                                        str(a.steps), "--warmup", str(a.warmup), "--data", data, "--model", a.model, "--stages", str(a.stages)])
                    if res is None:
                        return 1
                    res["round"] = rnd
                    log(res)
                    seen.setdefault(variant, []).append(res)
            if a.stages:
                sh = seen["shared"]
                keys = ("step_us", "order_us", "draw_us", "emit_single_us", "apply_us", "stages_sum_us", "emit_us")
                summary = dict(tool="shared_transd_timing", model=a.model, stages_summary=shape, chunk=chunk, rounds=a.rounds, batch=sh[0]["batch"],
                               negatives=sh[0]["negatives"], records=sh[-1]["records"], records_keyed=sh[-1]["records_keyed"])
                for k in keys:
                    summary[k], summary[k + "_range"] = med(sh, k), rng_(sh, k)
                log(summary)
                continue
            parent, sh = seen["parent"], seen["shared"]
            lo, hi = rng_(parent, "step_us")
            log(dict(tool="shared_transd_timing", model=a.model, summary=shape, chunk=chunk, rounds=a.rounds, batch=parent[0]["batch"],
                     negatives=parent[0]["negatives"], parent_step_us=med(parent, "step_us"), parent_step_us_range=[lo, hi],
                     unshared_step_us=med(seen["unshared"], "step_us"), unshared_step_us_range=rng_(seen["unshared"], "step_us"),
                     unshared_within_parent_range=bool(lo <= med(seen["unshared"], "step_us") <= hi),
                     shared_step_us=med(sh, "step_us"), shared_step_us_range=rng_(sh, "step_us"),
                     shared_step_ratio_to_parent=round(med(sh, "step_us") / med(parent, "step_us"), 3),
                     emit_us=med(sh, "emit_us"), emit_us_range=rng_(sh, "emit_us"), n_chunks=sh[-1]["n_chunks"],
                     chunk_ratio=med(sh, "chunk_ratio"), masked_share=med(sh, "masked_share"),
                     rows_gathered_ratio=round(sh[-1]["rows_gathered"] / sh[-1]["rows_gathered_unshared"], 4)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
