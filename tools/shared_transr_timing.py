#!/usr/bin/env python3
"""What TransR on shared negatives over RELATION-GROUPED chunks (Config.set_shared_negatives(..., by_relation=True) with the TransR
model; NON-PARITY, opt-in) costs against the unshared TransR step, on one MI355X.  Modelled on tools/shared_transd_timing.py.

The FB15k-237-shaped typed graph synthetic.FB15K237_TYPED (E = 14 541, R = 237, type_constrain.txt), De = Dr = 200, SGD, Bernoulli
sides, N = 25, type-constrained sampling on in every variant, at two batch sizes:
  headline  B = 34 014 (8 batches per epoch)
  small     B = 2 721 (100 batches per epoch: the reference's own batch)
Per shape, at equal B and N:
  parent    the unshared TransR step of the built checkout in --baseline-root: the baseline
  unshared  the same step from this tree (must lie within the parent's own round-to-round range: its path is untouched)
  shared    chunks by relation of P = 16 and P = 64: 2 P + N rows per chunk through the row GEMMs instead of P (2 + N)
and per shared case n_chunks / ceil(B / P) counted on the last step, the share of masked pairs and the GEMM rows (2 B + n_chunks N
live rows of the 2 B + cap N in the job list, against 2 B (1 + N) minus the alias rows of the unshared step).

--stages 1 is a run of its own: per (shape, P) one child per round times the stages of the shared step with device events, each
over 20 launches after 3 on the last step's inputs: order (kge_shared_order_by_relation), draw
(kge_shared_negatives_draw_grouped), the entry point stopped behind its first k stages for k = 1 .. 5 (option
shared_transr_stages: job list, projection, pair walk, dgrad, wgrad -- a stage's time is the difference of two such medians), and
the update (Config.apply_gradients, SGD on the whole tables), beside the whole step.

The engine is one per process, so every measurement is a child process of this driver with a time limit of its own; the driver
alternates the variants over --rounds rounds, stops at the first child that fails, and appends one JSON line per child and one
summary line per (shape, P) -- medians and ranges -- to --out (default profiles/shared_transr.jsonl).
Step time: host clock around --steps steps that end in a device synchronise, after --warmup steps.  Convergence is not measured.

usage: shared_transr_timing.py [--stages 1] [--shapes headline,small] [--rounds 3] [--steps 50] [--warmup 10] [--limit 300]
                               [--out FILE] [--baseline-root DIR] [--data DIR]"""
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
SHAPES = {"headline": dict(D=200, nbatches=8, n=25, chunks=(16, 64)), "small": dict(D=200, nbatches=100, n=25, chunks=(16, 64))}
STAGES = ("jobs", "project", "walk", "dgrad", "wgrad")


def configure(ok, a, s, shared):
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(s["D"]); con.set_ent_neg_rate(s["n"]); con.set_rel_neg_rate(0)
    con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method("SGD"); con.set_nbatches(s["nbatches"])
    if shared:
        con.set_shared_negatives(a.chunk, seed=1, by_relation=True)
    con.set_in_path(a.data)      # a dataset directory with type_constrain.txt
    con.set_type_constrained_sampling(True)
    con.init()
    con.set_model_and_session(ok.TransR)
    return con


def child(a):
    sys.path.insert(0, a.root)
    import torch
    import openkeonspark_amd as ok
    from openkeonspark_amd import _lib
    s = SHAPES[a.shape]
    shared = a.variant == "shared"
    con = configure(ok, a, s, shared)
    assert not con.sparse_inplace and not con.sparse_rows
    for _ in range(a.warmup):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = con.train_step(sync=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B, n, P = con.batch_size, s["n"], a.chunk
    res = dict(tool="shared_transr_timing", model="TransR", shape=a.shape, chunk=P, variant=a.variant, entities=con.entTotal, relations=con.relTotal,
               dim=s["D"], batch=B, negatives=n, steps=a.steps, step_us=round(dt / a.steps * 1e6, 2), loss=float(loss.item()))
    if shared:
        L, st, buf = con.lib, con._stream(), con._sparse_buf
        cand, pair, perm, chunks = con.shared_negatives_of(con.global_step - 1)
        cap = buf["shared_shape"][1]
        res["n_chunks"], res["chunks_by_position"], res["cap"] = len(chunks), -(-B // P), int(cap)
        res["chunk_ratio"] = round(len(chunks) / -(-B // P), 4)
        res["masked_share"] = round(float(((pair & 2) != 0).mean()), 6)
        res["gemm_rows"], res["job_list_rows"], res["gemm_rows_unshared_max"] = 2 * B + len(chunks) * n, 2 * B + int(cap) * n, 2 * B * (1 + n)
        if a.stages:
            h2, t2, r2 = (buf["sorted"][i].data_ptr() for i in range(3))
            dev = buf["shared_batch"]
            h, t, r = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
            step = con.global_step - 1

            def timed(fn):
                """median us per launch over 20 launches after 3"""
                out = []
                for i in range(23):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= 3:
                        out.append(e0.elapsed_time(e1))
                return round(statistics.median(out) * 1e3, 2)

            def entry():
                _lib.check(L.kge_transr_forward_backward_shared_chunks(
                    ctypes.byref(con._desc), con._tab_ptrs, h2, t2, r2, B, B, buf["chunks"].data_ptr(), cap, buf["cand"].data_ptr(), n,
                    buf["pair"].data_ptr(), B * n, con._grad_ptrs, con._loss.data_ptr(), st), L)

            res["order_us"] = timed(lambda: _lib.check(L.kge_shared_order_by_relation(
                h, t, r, B, P, buf["perm"].data_ptr(), h2, t2, r2, buf["chunks"].data_ptr(), buf["n_chunks"].data_ptr(), st), L))
            res["draw_us"] = timed(lambda: _lib.check(L.kge_shared_negatives_draw_grouped(
                h2, t2, r2, B, buf["chunks"].data_ptr(), cap, n, 1, con._shared_seed, step, buf["cand"].data_ptr(), buf["pair"].data_ptr(), st), L))
            before = 0.0
            for k, name in enumerate(STAGES, 1):      # the entry point stopped behind stage k: a stage is the difference
                L.kge_set_option(b"shared_transr_stages", k)
                upto = timed(entry)
                res[name + "_us"], before = round(upto - before, 2), upto
            res["entry_us"] = before
            res["update_us"] = timed(con.apply_gradients)      # (also zeroes the gradient tables the timed entries filled)
            res["stages_sum_us"] = round(res["order_us"] + res["draw_us"] + res["entry_us"] + res["update_us"], 2)
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
    ap.add_argument("--shapes", default="headline,small")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_transr.jsonl"))
    ap.add_argument("--stages", type=int, default=0, help="1: time the shared step's stages one by one instead of the variants")
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
    base = a.data or tempfile.mkdtemp(prefix="shared_transr_")
    data = synthetic.make_typed_dataset(os.path.join(base, "fb15k237_typed"), synthetic.FB15K237_TYPED)

    def log(res):
        print(json.dumps(res), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")

    med = lambda rs, k: statistics.median(x[k] for x in rs)
    rng_ = lambda rs, k: [min(x[k] for x in rs), max(x[k] for x in rs)]
    for shape in [x for x in a.shapes.split(",") if x]:
        chunks = SHAPES[shape]["chunks"]
        variants = [("shared", c) for c in chunks] if a.stages else [("parent", 0), ("unshared", 0)] + [("shared", c) for c in chunks]
        seen = {}
        for rnd in range(a.rounds):
            for variant, chunk in variants:
                root = a.baseline_root if variant == "parent" else ROOT
                res = run_child(a, ["--child", "--shape", shape, "--chunk", str(chunk), "--variant", variant, "--root", root, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup), "--data", data, "--stages", str(a.stages)])
                if res is None:
                    return 1
                res["round"] = rnd
                log(res)
                seen.setdefault((variant, chunk), []).append(res)
        for chunk in chunks:
            sh = seen["shared", chunk]
            if a.stages:
                keys = ("step_us", "order_us", "draw_us") + tuple(k + "_us" for k in STAGES) + ("entry_us", "update_us", "stages_sum_us")
                summary = dict(tool="shared_transr_timing", model="TransR", stages_summary=shape, chunk=chunk, rounds=a.rounds, batch=sh[0]["batch"],
                               negatives=sh[0]["negatives"], gemm_rows=sh[-1]["gemm_rows"], job_list_rows=sh[-1]["job_list_rows"])
                for k in keys:
                    summary[k], summary[k + "_range"] = med(sh, k), rng_(sh, k)
                log(summary)
                continue
            parent, un = seen["parent", 0], seen["unshared", 0]
            lo, hi = rng_(parent, "step_us")
            log(dict(tool="shared_transr_timing", model="TransR", summary=shape, chunk=chunk, rounds=a.rounds, batch=parent[0]["batch"],
                     negatives=parent[0]["negatives"], parent_step_us=med(parent, "step_us"), parent_step_us_range=[lo, hi],
                     unshared_step_us=med(un, "step_us"), unshared_step_us_range=rng_(un, "step_us"),
                     unshared_within_parent_range=bool(lo <= med(un, "step_us") <= hi),
                     shared_step_us=med(sh, "step_us"), shared_step_us_range=rng_(sh, "step_us"),
                     shared_step_ratio_to_parent=round(med(sh, "step_us") / med(parent, "step_us"), 3), n_chunks=sh[-1]["n_chunks"],
                     chunk_ratio=med(sh, "chunk_ratio"), masked_share=med(sh, "masked_share"), gemm_rows=sh[-1]["gemm_rows"],
                     job_list_rows=sh[-1]["job_list_rows"], gemm_rows_unshared_max=sh[-1]["gemm_rows_unshared_max"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
