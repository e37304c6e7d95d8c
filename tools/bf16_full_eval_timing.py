#!/usr/bin/env python3
"""What the full-entity evaluators cost on stored bf16 tables (kge_rank_triples_bf16, kge_topk_entities_bf16), on one MI355X.
The sibling of bf16_eval_timing.py, which measures the evaluators that gather rows.

Shape: the 5 M x 200 TransE table of DESIGN 4.8 / 4.9 (2 GB stored as bf16, 4 GB as float32), uniform random triples.
  rank   Config.rank_triples on 2 000 triples, both sides (every entity a candidate)
  topk   Config.top_k_tails on 4 096 queries, k = 10, filtered
each in these arms:
  stored        bf16 tables, set_bf16_evaluation("stored"): the bf16 kernels on the stored rows, no view, no candidate table
  view_rebuilt  bf16 tables; every call widens both tables into a fresh float32 view and runs the fp32 path on it -- what a
                check met before the stored path (a training step drops the view).  With --baseline-root this arm runs in that
                built checkout: the parent commit's own code
  view_cached   bf16 tables; the fp32 path on a view made once, outside the clock
  fp32_tables   fp32 tables and the fp32 path (with --baseline-root also in that checkout: the fp32 path must not move)

The engine is one per process, so every arm is a child process of this driver with a time limit of its own; the children are
alternated over --rounds rounds and the driver stops at the first child that fails.  A child times --reps calls between device
events after --warmup calls and reports the median, the rise of torch.cuda.max_memory_allocated over the timed and warm-up calls
and the peak rise of kge_workspace_bytes (null where the checkout has no such call).  One JSON line per (child, call) is appended
to --out (default profiles/bf16_full_eval.jsonl); the driver ends with one summary line per (call, arm, checkout).

usage: bf16_full_eval_timing.py [--what rank,topk] [--rounds 3] [--reps 10] [--warmup 2] [--limit 400] [--out FILE]
                                [--baseline-root DIR] [--entities 5000000] [--dim 200]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, TRAIN, N_RANK, N_TOPK, K = 1000, 2_000_000, 2_000, 4_096, 10
ARMS = ("stored", "view_rebuilt", "view_cached", "fp32_tables")


def child(a):
    sys.path.insert(0, a.root)
    import ctypes
    import numpy as np
    import torch
    import openkeonspark_amd as ok
    E, D = a.entities, a.dim
    rng = np.random.default_rng(5)
    draw = lambda n: (rng.integers(0, E, n, dtype=np.int64), rng.integers(0, E, n, dtype=np.int64), rng.integers(0, R, n, dtype=np.int64))
    con = ok.Config()
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(D); con.set_ent_neg_rate(1); con.set_rel_neg_rate(0)
    con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method("SGD"); con.set_nbatches(100)
    con.sparse_rows = True
    if a.arm != "fp32_tables":
        con.set_table_dtype("bf16", seed=1)
    con.init_from_arrays(E, R, *draw(TRAIN))
    valid = draw(N_RANK)
    con.init_evaluation_from_arrays(valid, draw(1000))
    con.set_model_and_session(ok.TransE)
    if a.arm == "stored":
        con.set_bf16_evaluation("stored")
    table_bytes = sum(t.numel() * t.element_size() for t in con._tables)
    counted = hasattr(con.lib, "kge_workspace_bytes")

    def workspace(reset):
        if not counted:
            return None, None
        live, peak = ctypes.c_int64(), ctypes.c_int64()
        con.lib.kge_workspace_bytes(ctypes.byref(live), ctypes.byref(peak), reset)
        return live.value, peak.value

    qh, _, qr = draw(N_TOPK)
    calls = {"rank": lambda: con.rank_triples(*valid)[0], "topk": lambda: con.top_k_tails(qh, qr, K, filtered=True)[0]}
    for what in a.what.split(","):
        def call():
            if a.arm == "view_rebuilt":
                con._drop_eval_view()
            return calls[what]()
        con._drop_eval_view()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        live0, _ = workspace(1)
        for _ in range(a.warmup):
            call()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = call(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        rise = int(torch.cuda.max_memory_allocated()) - base
        _, peak = workspace(0)
        res = dict(tool="bf16_full_eval_timing", what=what, arm=a.arm, root="this tree" if os.path.abspath(a.root) == ROOT else "baseline",
                   entities=E, dim=D, reps=a.reps, ms=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                   table_bytes=table_bytes, torch_peak_rise=rise, workspace_peak_rise=None if peak is None else peak - live0,
                   view=con._eval_view is not None, checksum=float(np.asarray(out, dtype=np.float64).sum()),
                   **(dict(triples=N_RANK, sides=2) if what == "rank" else dict(queries=N_TOPK, k=K)))
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
    ap.add_argument("--what", default="rank,topk")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_full_eval.jsonl"))
    ap.add_argument("--baseline-root", default="")
    ap.add_argument("--entities", type=int, default=5_000_000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--child", default="")
    ap.add_argument("--arm", default="stored")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        a.what = a.child
        return child(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    base = a.baseline_root
    variants = [(ROOT, "stored"), (base or ROOT, "view_rebuilt"), (ROOT, "view_cached"), (ROOT, "fp32_tables")] + ([(base, "fp32_tables")] if base else [])
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
        ws = [r["workspace_peak_rise"] for r in rs if r["workspace_peak_rise"] is not None]
        print("SUMMARY " + json.dumps(dict(what=what, arm=arm, root=root, rounds=len(ms), ms_median=statistics.median(ms), ms_min=min(ms),
                                            ms_max=max(ms), torch_peak_rise=max(r["torch_peak_rise"] for r in rs),
                                            workspace_peak_rise=max(ws) if ws else None,
                                            checksums_agree=len({r["checksum"] for r in rs}) == 1)), flush=True)
    for what in sorted({k[0] for k in seen}):      # the readings of the bf16 tables must have computed the same thing
        sums = {"%s (%s)" % (arm, root): rs[0]["checksum"] for (w, arm, root), rs in seen.items() if w == what and arm != "fp32_tables"}
        print("SUMMARY " + json.dumps(dict(what=what, bf16_table_checksums=sums, agree=len(set(sums.values())) == 1)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
