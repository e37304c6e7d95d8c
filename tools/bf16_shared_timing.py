#!/usr/bin/env python3
"""What shared negatives on bf16 tables (Config.set_table_dtype("bf16") with Config.set_shared_negatives; NON-PARITY, opt-in) cost
and save, on one MI355X.

Two HBM-resident shapes, TransE on sparse rows, Bernoulli sides, uniform random triples, chunks by position:
  e5m_d200  the 5 M x 200 table (4 GB in fp32) of DESIGN 4.8: 8 M triples, B = 131 147, n = 25, P = 16 and 64
  e5m_d512  a 5 M x 512 table (10 GB in fp32): 8 M triples, B = 131 147, n = 1, P = 64
each with SGD and with RowAdagrad, in three variants: the fp32 shared step of --baseline-root (a built checkout of the commit this
one is compared with), the fp32 shared step of this tree, and the bf16 shared step of this tree.

The engine is one per process, so every (shape, chunk, optimizer, variant) is a child process of this driver with a time limit of
its own; the driver runs them one after the other and stops at the first child that fails.  A child runs --rounds rounds of
--steps steps (host clock around steps that end in a device synchronise, after --warmup steps) and reports the median and the
range over the rounds; then, on the last step's batch and lists, device events around 20 launches of each stage -- draw, emit,
reduce, apply -- after 3 warm-up launches (the fp32 SGD step fuses reduce and apply; its variants time the unfused pair beside
the step they run), and torch.cuda.max_memory_allocated.  One JSON line per child is appended to --out (default
profiles/bf16_shared.jsonl).

usage: bf16_shared_timing.py [--shapes e5m_d200,e5m_d512] [--optimizers SGD,RowAdagrad] [--rounds 3] [--steps 50] [--warmup 5]
                             [--limit 300] [--out FILE] [--baseline-root DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"e5m_d200": dict(E=5_000_000, R=1000, D=200, triples=8_000_000, nbatches=61, n=25, chunks=(16, 64)),
          "e5m_d512": dict(E=5_000_000, R=1000, D=512, triples=8_000_000, nbatches=61, n=1, chunks=(64,))}


def child(a):
    sys.path.insert(0, a.root)
    import ctypes
    import numpy as np
    import torch
    import openkeonspark_amd as ok
    from openkeonspark_amd import _lib
    s = SHAPES[a.shape]
    bf16 = a.dtype == "bf16"
    P = a.chunk
    rng = np.random.default_rng(5)
    h = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
    t = rng.integers(0, s["E"], s["triples"], dtype=np.int64)
    r = rng.integers(0, s["R"], s["triples"], dtype=np.int64)
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(s["D"]); con.set_ent_neg_rate(s["n"]); con.set_rel_neg_rate(0)
    con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method(a.optimizer); con.set_nbatches(s["nbatches"])
    con.sparse_rows = True
    con.set_shared_negatives(P, seed=1)
    if bf16:
        con.set_table_dtype("bf16", seed=2)      # (not the shared-negatives seed: equal seeds are refused)
    con.init_from_arrays(s["E"], s["R"], h, t, r)
    del h, t, r
    con.set_model_and_session(ok.TransE)
    assert con.sparse_rows
    for _ in range(a.warmup):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    step_us = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = con.train_step(sync=False)
        torch.cuda.synchronize()
        step_us.append(round((time.perf_counter() - t0) / a.steps * 1e6, 2))
    B, n, D = con.batch_size, s["n"], s["D"]
    n_chunks = -(-B // P)
    width = 2 if bf16 else 4
    res = dict(tool="bf16_shared_timing", shape=a.shape, chunk=P, optimizer=a.optimizer, table_dtype=a.dtype,
               root="this tree" if os.path.abspath(a.root) == ROOT else "baseline", entities=s["E"], dim=D, batch=B, negatives=n,
               rounds=a.rounds, steps=a.steps, step_us=statistics.median(step_us), step_us_rounds=step_us, loss=float(loss.item()),
               gather_bytes=(3 * B + n_chunks * n) * D * width, table_bytes=sum(t.numel() * t.element_size() for t in con._tables))
    # the stages alone, on the last step's batch and lists
    L, st, buf, desc = con.lib, con._stream(), con._sparse_buf, ctypes.byref(con._desc)
    dev = buf["shared_batch"]
    hp, tp, rp = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
    ent, rel = con._tables[0].data_ptr(), con._tables[1].data_ptr()
    M = 3 * B + n_chunks * n
    ptr = lambda k: buf[k].data_ptr()
    ada = a.optimizer == "RowAdagrad"
    acc = [x.data_ptr() for x in con._rowadagrad_acc] if ada else []
    loss_buf = torch.zeros(1, dtype=torch.float32, device=con.device)
    step_no = con.global_step - 1

    def draw():
        _lib.check(L.kge_shared_negatives_draw(hp, tp, rp, B, 0, P, n, con._shared_seed, step_no, ptr("cand"), ptr("pair"), st), L)

    def emit():
        call = L.kge_transe_emit_records_shared_bf16 if bf16 else L.kge_transe_emit_records_shared
        _lib.check(call(desc, ent, rel, hp, tp, rp, B, B, P, ptr("cand"), n, ptr("pair"), B * n, ptr("rec"), ptr("dst"), loss_buf.data_ptr(), st), L)

    def reduce():
        _lib.check(L.kge_transe_reduce_records(desc, ptr("rec"), ptr("dst"), M, ptr("rows"), ptr("row_counts"), ptr("n_rows"), st), L)

    def apply():      # (lr = 0: the tables the next launch reads are the ones this one read)
        if bf16 and ada:
            _lib.check(L.kge_transe_apply_rows_rowadagrad_bf16(desc, ent, rel, *acc, ptr("rows"), ptr("row_counts"), ptr("n_rows"), M, B * n,
                                                               0.0, ctypes.c_uint64(1), ctypes.c_uint64(0), st), L)
        elif bf16:
            _lib.check(L.kge_transe_apply_rows_sgd_bf16(desc, ent, rel, ptr("rows"), ptr("row_counts"), ptr("n_rows"), M, B * n, 0.0,
                                                        ctypes.c_uint64(1), ctypes.c_uint64(0), st), L)
        elif ada:
            _lib.check(L.kge_transe_apply_rows_rowadagrad(desc, ent, rel, *acc, ptr("rows"), ptr("row_counts"), ptr("n_rows"), M, B * n, 0.0, st), L)
        else:
            _lib.check(L.kge_transe_apply_rows_sgd(desc, ent, rel, ptr("rows"), ptr("row_counts"), ptr("n_rows"), M, B * n, 0.0, st), L)

    def timed(call, before=None):
        us = []
        for i in range(23):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                us.append(e0.elapsed_time(e1) * 1e3)
        return round(statistics.median(us), 2)
    res["draw_us"] = timed(draw)
    res["emit_us"] = timed(emit)      # (with the loss kernel behind it: one block)
    res["reduce_us"] = timed(reduce, before=emit)      # (the reduce overwrites the keys: every launch gets fresh ones)
    emit(); reduce()
    res["apply_us"] = timed(apply)
    res["emit_gather_GBps"] = round(res["gather_bytes"] / (res["emit_us"] * 1e-6) / 1e9, 1)
    res["max_memory_allocated"] = int(torch.cuda.max_memory_allocated())
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
    ap.add_argument("--shapes", default="e5m_d200,e5m_d512")
    ap.add_argument("--optimizers", default="SGD,RowAdagrad")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_shared.jsonl"))
    ap.add_argument("--baseline-root", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default="e5m_d200")
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--optimizer", default="SGD")
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    variants = ([(a.baseline_root, "fp32")] if a.baseline_root else []) + [(ROOT, "fp32"), (ROOT, "bf16")]
    for shape in [s for s in a.shapes.split(",") if s]:
        for chunk in SHAPES[shape]["chunks"]:
            for opt in a.optimizers.split(","):
                for root, dtype in variants:
                    res = run_child(a, ["--child", "--shape", shape, "--chunk", str(chunk), "--optimizer", opt, "--dtype", dtype, "--root", root,
                                        "--rounds", str(a.rounds), "--steps", str(a.steps), "--warmup", str(a.warmup)])
                    if res is None:
                        return 1
                    print(json.dumps(res), flush=True)
                    with open(a.out, "a") as f:
                        f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
