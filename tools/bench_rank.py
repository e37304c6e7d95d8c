#!/usr/bin/env python3
"""kge_rank_triples against kge_link_prediction on the same triples in the same process: the FB15k-237-shaped synthetic KG of
bench_lp.py (20 466 test / 17 535 validation triples, 14 541 entities), both sides.  After a warm-up, five timed repetitions
each of link_prediction() (the baseline: code the fused ranker does not touch), rank_triples on the test triples in the same
order, and validation_link_prediction().  Appends one JSON line to profiles/rank_triples.jsonl (or --out).
usage: bench_rank.py [MODEL] [DIM] [--out FILE] [--reps N]
Exits non-zero when the counts differ from link_prediction's.
Kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_rank.py MODEL DIM --reps 1"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from bench_lp import dataset      # the same graph in the same cache directory


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out, res


def summary(ts):
    return {"min_ms": round(1e3 * min(ts), 3), "median_ms": round(1e3 * float(np.median(ts)), 3), "max_ms": round(1e3 * max(ts), 3),
            "all_ms": [round(1e3 * x, 3) for x in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="TransE")
    ap.add_argument("dim", nargs="?", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_triples.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import openkeonspark_amd as pkg
    d = dataset()
    con = pkg.Config()
    con.set_in_path(d); con.set_work_threads(8); con.set_bern(1); con.set_dimension(a.dim); con.set_nbatches(8)
    con.set_ent_neg_rate(25); con.set_alpha(0.001); con.set_opt_method("Adam")
    con.init()
    con.init_link_prediction()
    con.set_model_and_session(getattr(pkg, a.model))
    for _ in range(30):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    with open(d + "test2id.txt") as f:
        tok = f.read().split()
    tt = np.asarray(tok[1:], dtype=np.int64).reshape(-1, 3)
    tt = tt[np.lexsort((tt[:, 1], tt[:, 0], tt[:, 2]))]          # link_prediction's order: (r, h, t)
    # warm-up: the filter upload, every workspace, the cached validation ids
    con.link_prediction(0, 256)
    con.rank_triples(tt[:256, 0], tt[:256, 1], tt[:256, 2])
    con.validation_link_prediction()
    base, (lp_out, lp_met) = timed(con.link_prediction, a.reps)
    rank, (counts, met) = timed(lambda: con.rank_triples(tt[:, 0], tt[:, 1], tt[:, 2]), a.reps)
    valid, (vcounts, vmet) = timed(con.validation_link_prediction, a.reps)
    line = {"model": a.model, "dim": a.dim, "entities": con.entTotal, "test_triples": int(tt.shape[0]), "valid_triples": int(vcounts.shape[0]),
            "link_prediction": summary(base), "rank_triples_test": summary(rank), "validation_link_prediction": summary(valid),
            "baseline_spread_ms": round(1e3 * (max(base) - min(base)), 3),
            "rank_minus_baseline_median_ms": round(1e3 * float(np.median(rank) - np.median(base)), 3),
            "counts_equal_link_prediction": bool(np.array_equal(counts, lp_out[:, :, :4])),
            "MRR_filter_tail_test": met["r_filter_reci_rank"], "MRR_filter_tail_valid": vmet["r_filter_reci_rank"]}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    if not line["counts_equal_link_prediction"]:
        sys.exit("rank_triples' counts differ from link_prediction's columns 0..3")


if __name__ == "__main__":
    main()
