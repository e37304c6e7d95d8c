#!/usr/bin/env python3
"""What training on shared negatives (Config.set_shared_negatives; NON-PARITY, opt-in) costs and saves, on one MI355X.

Two shapes, TransE with SGD on sparse rows, Bernoulli sides, uniform random triples:
  headline  E = 14 541, R = 237, D = 200, B = 34 014, n = 25 (the benchmark's batch)
  large     the 5 M x 200 table (4 GB) of DESIGN 4.8: 8 M triples, B = 131 147, n = 25
For each: the per-step time of the shared step at chunks of P = 16, 64, 127 positives, the unshared sparse-rows step at the same
B and n, the shared emit kernel's own time, and the algorithmic gather bytes of both emit stages per step:
  unshared  B (3 + n) D 4           shared  (3 B + ceil(B / P) n) D 4

The engine is one per process, so every measurement is a child process of this driver, with a time limit of its own; the driver
alternates the variants over --rounds rounds, stops at the first child that fails, and appends one JSON line per child to --out
(default profiles/shared_negatives.jsonl) and a summary line (medians and ranges) at the end.  --baseline-root DIR: the unshared
step is measured from the built checkout in DIR (the commit this one is compared with) instead of from this tree.
Step time: host clock around --steps steps that end in a device synchronise, after --warmup steps.  Kernel time: device events
around 20 launches of kge_transe_emit_records_shared on the last step's lists, after 3 warm-up launches.

usage: shared_negatives_timing.py [--shapes headline,large] [--rounds 3] [--steps 100] [--warmup 10] [--limit 300] [--out FILE]
                                  [--baseline-root DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"headline": dict(E=14541, R=237, D=200, triples=272115, nbatches=8, n=25),
          "large": dict(E=5_000_000, R=1000, D=200, triples=8_000_000, nbatches=61, n=25)}
CHUNKS = (16, 64, 127)


def child(a):
    sys.path.insert(0, a.root)
    import ctypes
    import numpy as np
    import torch
    import openkeonspark_amd as ok
    from openkeonspark_amd import _lib
    s = SHAPES[a.shape]
    rng = np.random.default_rng(5)
    h = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
    t = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
    r = rng.integers(0, s["R"], s["triples"], dtype=np.int64)
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(s["D"]); con.set_ent_neg_rate(s["n"]); con.set_rel_neg_rate(0)
    con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method("SGD"); con.set_nbatches(s["nbatches"])
    con.sparse_rows = True
    if a.chunk:
        con.set_shared_negatives(a.chunk, seed=1)
    con.init_from_arrays(s["E"], s["R"], h, t, r)
    del h, t, r
    con.set_model_and_session(ok.TransE)
    assert con.sparse_rows
    for _ in range(a.warmup):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = con.train_step(sync=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    B, n, D = con.batch_size, s["n"], s["D"]
    res = dict(tool="shared_negatives_timing", shape=a.shape, chunk=a.chunk, root="this tree" if os.path.abspath(a.root) == ROOT else "baseline",
               entities=s["E"], dim=D,
               batch=B, negatives=n, steps=a.steps, step_us=round(dt / a.steps * 1e6, 2), loss=float(loss.item()),
               gather_bytes=(3 * B + -(-B // a.chunk) * n) * D * 4 if a.chunk else B * (3 + n) * D * 4)
    if a.chunk:      # the emit kernel alone, on the last step's lists
        buf, dev = con._sparse_buf, con._sparse_buf["shared_batch"]
        loss_buf = torch.zeros(1, dtype=torch.float32, device=con.device)

        def emit():
            _lib.check(con.lib.kge_transe_emit_records_shared(
                ctypes.byref(con._desc), con._tables[0].data_ptr(), con._tables[1].data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(),
                dev[2].data_ptr(), B, B, a.chunk, buf["cand"].data_ptr(), n, buf["pair"].data_ptr(), B * n, buf["rec"].data_ptr(),
                buf["dst"].data_ptr(), loss_buf.data_ptr(), con._stream()), con.lib)
        for _ in range(3):
            emit()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            emit()
        e1.record()
        torch.cuda.synchronize()
        res["emit_us"] = round(e0.elapsed_time(e1) / 20 * 1e3, 2)      # (with the loss kernel behind it: one block)
        res["emit_gather_GBps"] = round(res["gather_bytes"] / (res["emit_us"] * 1e-6) / 1e9, 1)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,large")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_negatives.jsonl"))
    ap.add_argument("--baseline-root", default=ROOT)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default="headline")
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in a.shapes.split(","):
        seen = {}
        for rnd in range(a.rounds):
            for chunk in (0,) + CHUNKS:
                root = a.baseline_root if chunk == 0 else ROOT
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", shape, "--chunk", str(chunk), "--root", root,
                       "--steps", str(a.steps), "--warmup", str(a.warmup)]
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    print("child %s ran into its limit of %d s: stopping" % (cmd[3:9], a.limit), file=sys.stderr)
                    return 2
                lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    print("child %s failed (exit %d): stopping\n%s" % (cmd[3:9], p.returncode, p.stderr[-2000:]), file=sys.stderr)
                    return p.returncode or 1
                res = json.loads(lines[-1][7:])
                res["round"] = rnd
                print(json.dumps(res), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(res) + "\n")
                seen.setdefault(chunk, []).append(res)
        med = lambda rs, k: statistics.median(x[k] for x in rs)
        rng_ = lambda rs, k: [min(x[k] for x in rs), max(x[k] for x in rs)]
        base = seen[0]
        summary = dict(tool="shared_negatives_timing", summary=shape, rounds=a.rounds, batch=base[0]["batch"], negatives=base[0]["negatives"],
                       unshared_from=base[0]["root"], unshared_step_us=med(base, "step_us"), unshared_step_us_range=rng_(base, "step_us"),
                       unshared_gather_bytes=base[0]["gather_bytes"])
        for chunk in CHUNKS:
            rs = seen[chunk]
            summary["P%d" % chunk] = dict(step_us=med(rs, "step_us"), step_us_range=rng_(rs, "step_us"), emit_us=med(rs, "emit_us"),
                                          emit_us_range=rng_(rs, "emit_us"), gather_bytes=rs[0]["gather_bytes"],
                                          step_ratio_to_unshared=round(med(rs, "step_us") / med(base, "step_us"), 3),
                                          gather_bytes_ratio=round(rs[0]["gather_bytes"] / base[0]["gather_bytes"], 3))
        print(json.dumps(summary), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(summary) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
