#!/usr/bin/env python3
"""What evaluating straight from bf16 tables (kge_rank_candidates_bf16, kge_predict_bf16) costs and saves, on one MI355X.

Shape: the 5 M x 200 TransE table of DESIGN 4.8 / 4.9 (2 GB stored as bf16, 4 GB as float32), uniform random triples.
  rank     an early-stop check: n = 20 000 validation triples against C = 1000 drawn candidates, filtered, both sides
  predict  test_step's call on 1 M triples
each in these arms:
  view_rebuilt  bf16 tables; every call widens both tables into a fresh float32 view and runs the fp32 kernel on it -- the check
                as a training loop met it before the bf16 entry points (a training step drops the view before every check)
  view_cached   bf16 tables; the fp32 kernel on a view made once, outside the clock
  bf16          bf16 tables; the bf16 kernel on the stored rows, no view
  fp32_tables   fp32 tables and the fp32 kernel (with --baseline-root also in that built checkout: the fp32 path must not move)

The engine is one per process, so every arm is a child process of this driver (it measures both calls) with a time limit of its
own; the children are alternated over --rounds rounds and the driver stops at the first child that fails.  A child times --reps
calls with device events after --warmup calls and reports the median, and torch.cuda.max_memory_allocated over the timed calls
beside the bytes the tables themselves take.  One JSON line per (child, call) is appended to --out (default
profiles/bf16_eval.jsonl); the driver ends with one summary line per (call, arm): the median and the range over the rounds.

usage: bf16_eval_timing.py [--what rank,predict] [--rounds 3] [--reps 10] [--warmup 2] [--limit 300] [--out FILE]
                           [--baseline-root DIR] [--entities 5000000] [--dim 200]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, TRAIN, N_RANK, C_RANK, N_PREDICT = 1000, 2_000_000, 20_000, 1000, 1_000_000
ARMS = ("view_rebuilt", "view_cached", "bf16", "fp32_tables")


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import openkeonspark_amd as ok
    E, D = a.entities, a.dim
    bf16 = a.arm != "fp32_tables"
    rng = np.random.default_rng(5)
    draw = lambda n: (rng.integers(0, E, n, dtype=np.int64), rng.integers(0, E, n, dtype=np.int64), rng.integers(0, R, n, dtype=np.int64))
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(D); con.set_ent_neg_rate(1); con.set_rel_neg_rate(0)
    con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method("SGD"); con.set_nbatches(100)
    con.sparse_rows = True
    if bf16:
        con.set_table_dtype("bf16", seed=1)
    con.init_from_arrays(E, R, *draw(TRAIN))
    valid = draw(N_RANK)
    con.init_evaluation_from_arrays(valid, draw(1000))
    con.set_model_and_session(ok.TransE)
    table_bytes = sum(t.numel() * t.element_size() for t in con._tables)
    raw = [t.data_ptr() for t in con._tables]
    for what in a.what.split(","):
        measure(a, con, what, valid, draw, table_bytes, raw)


def measure(a, con, what, valid, draw, table_bytes, raw):
    import ctypes
    import numpy as np
    import torch
    from openkeonspark_amd import _lib
    L, desc, st = con.lib, ctypes.byref(con._desc), con._stream()
    if what == "rank":
        ids = torch.from_numpy(np.stack(valid).astype(np.int32)).to(con.device)
        n = N_RANK
        out = torch.empty((n, 2, 2), dtype=torch.int64, device=con.device)
        flags = _lib.RANKC_FILTERED | _lib.RANKC_DRAWN
        tail = (ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n, None, 0, None, 0, C_RANK, flags, 7, out.data_ptr(), st)
        fp32_fn, bf16_fn = L.kge_rank_candidates, getattr(L, "kge_rank_candidates_bf16", None)
        work = dict(triples=n, candidates=C_RANK, gathered_rows=2 * n * (C_RANK + 2))
    else:
        ids = torch.from_numpy(np.stack(draw(N_PREDICT)).astype(np.int32)).to(con.device)
        n = N_PREDICT
        out = torch.empty(n, dtype=torch.float32, device=con.device)
        tail = (ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n, out.data_ptr(), st)
        fp32_fn, bf16_fn = L.kge_predict, getattr(L, "kge_predict_bf16", None)
        work = dict(triples=n, gathered_rows=3 * n)

    def call():
        if a.arm == "bf16":
            _lib.check(bf16_fn(desc, raw[0], raw[1], *tail), L)
        elif a.arm == "fp32_tables":
            _lib.check(fp32_fn(desc, con._tab_ptrs, *tail), L)
        else:
            if a.arm == "view_rebuilt":
                con._drop_eval_view()
            _lib.check(fp32_fn(desc, con._eval_table_ptrs(), *tail), L)

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    peak = int(torch.cuda.max_memory_allocated())
    if a.arm.startswith("view"):
        con._drop_eval_view()
    res = dict(tool="bf16_eval_timing", what=what, arm=a.arm, root="this tree" if os.path.abspath(a.root) == ROOT else "baseline",
               entities=a.entities, dim=a.dim, reps=a.reps, ms=round(statistics.median(ms), 3), ms_min=round(min(ms), 3),
               ms_max=round(max(ms), 3), table_bytes=table_bytes, max_memory_allocated=peak, above_tables_bytes=peak - table_bytes,
               checksum=float(out.double().sum().item()), **work)
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
    return [json.loads(l[7:]) for l in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="rank,predict")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_eval.jsonl"))
    ap.add_argument("--baseline-root", default="")
    ap.add_argument("--entities", type=int, default=5_000_000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--child", default="")
    ap.add_argument("--arm", default="bf16")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        a.what = a.child
        return child(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    variants = [(ROOT, arm) for arm in ARMS] + ([(a.baseline_root, "fp32_tables")] if a.baseline_root else [])
    seen = {}
    for rnd in range(a.rounds):
        for root, arm in variants:
            results = run_child(a, ["--child", a.what, "--arm", arm, "--root", root, "--reps", str(a.reps), "--warmup", str(a.warmup),
                                    "--entities", str(a.entities), "--dim", str(a.dim)])
            if results is None:
                return 1
            for res in results:
                res["round"] = rnd
                print(json.dumps(res), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(res) + "\n")
                seen.setdefault((res["what"], arm, res["root"]), []).append(res)
    for (what, arm, root), rs in seen.items():
        ms = [r["ms"] for r in rs]
        print("SUMMARY " + json.dumps(dict(what=what, arm=arm, root=root, rounds=len(ms), ms_median=statistics.median(ms), ms_min=min(ms),
                                            ms_max=max(ms), above_tables_bytes=max(r["above_tables_bytes"] for r in rs),
                                            checksums_agree=len({r["checksum"] for r in rs}) == 1)), flush=True)
    for what in sorted({k[0] for k in seen}):      # the three readings of the bf16 tables must have computed the same thing
        sums = {arm: seen[(what, arm, "this tree")][0]["checksum"] for arm in ARMS[:3] if (what, arm, "this tree") in seen}
        print("SUMMARY " + json.dumps(dict(what=what, bf16_table_checksums=sums, agree=len(set(sums.values())) == 1)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
