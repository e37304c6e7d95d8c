#!/usr/bin/env python3
"""kge_rank_candidates (drawn lists) in its fused and its two-stage form, and kge_rank_triples on the same triples where the
full ranking fits, in one process: five interleaved rounds after a warm-up, host clock around synchronised calls.
  fb     the FB15k-237-shaped synthetic KG of bench_lp.py: E = 14 541, the 20 466 test triples, C = 1000, both sides
  large  a table beyond the Infinity Cache: E = 5 000 000 x D, 100 000 random triples, C = 500, both sides (no full ranking)
Appends one JSON line to profiles/rank_candidates.jsonl (or --out) with the median / min / max ms of each form and the
algorithmic gather rate n x sides x C x D x 4 B / median time.
usage: bench_rank_candidates.py [fb|large] [MODEL] [DIM] [--out FILE] [--rounds N] [--candidates C]
Exits non-zero when the two forms' counts differ.
  --range-cut W [W ...]   (large, TransE) what one rank of a W-way sharded table pays: kge_rank_candidates_range on the first 1/W of
the rows against kge_rank_candidates on the whole table, the same triples and drawn lists, both on device-resident ids and
counts; the query rows are prepared outside the timed region.  One JSON line per W; exits non-zero when the W ranges' counts do
not sum to the whole table's."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np


def summary(ts):
    return {"min_ms": round(1e3 * min(ts), 3), "median_ms": round(1e3 * float(np.median(ts)), 3), "max_ms": round(1e3 * max(ts), 3),
            "all_ms": [round(1e3 * x, 3) for x in ts]}


def fb_engine(pkg, model, dim):
    from bench_lp import dataset      # the same graph in the same cache directory
    d = dataset()
    con = pkg.Config()
    con.set_in_path(d); con.set_work_threads(8); con.set_bern(1); con.set_dimension(dim); con.set_nbatches(8)
    con.set_ent_neg_rate(25); con.set_alpha(0.001); con.set_opt_method("Adam")
    con.init()
    con.init_link_prediction()
    con.set_model_and_session(getattr(pkg, model))
    for _ in range(30):
        con.train_step(sync=False)
    with open(d + "test2id.txt") as f:
        tok = f.read().split()
    tt = np.asarray(tok[1:], dtype=np.int64).reshape(-1, 3)
    return con, tt


def large_engine(pkg, model, dim, entities, triples):
    rng = np.random.default_rng(1)
    R = 500
    draw = lambda n: (rng.integers(0, entities, n), rng.integers(0, entities, n), rng.integers(0, R, n))
    con = pkg.Config()
    con.set_work_threads(8); con.set_dimension(dim); con.set_nbatches(100)
    con.init_from_arrays(entities, R, *draw(200000))
    con.set_model_and_session(getattr(pkg, model))
    for t in con._tables:                       # spread the scores: freshly initialised tables rank almost at random
        t.mul_(3.0)
    con.tables_changed()
    con.init_evaluation_from_arrays(draw(1000), draw(1000))
    return con, np.stack(draw(triples), 1)


def range_cut(con, tt, C, W, rounds, seed=1):
    """-> the JSON line of one W: the range call on rows [0, ceil(E / W)) and the whole-table call, interleaved."""
    import torch
    from openkeonspark_amd import _lib, rank_eval
    E, D, L, st = con.entTotal, con.hidden_size, con.lib, con._stream()
    ent, rel = con._tables[0], con._tables[1]
    flags = _lib.RANKC_DRAWN | _lib.RANKC_FILTERED
    ids = torch.from_numpy(np.ascontiguousarray(tt.T.astype(np.int32))).to(con.device)
    n = ids.shape[1]
    query = ent.index_select(0, ids[:2].t().reshape(-1).long()).contiguous()      # [n][2][D], outside the timed region
    chunk = -(-E // W)
    whole_counts = torch.empty((n, 2, 2), dtype=torch.int64, device=con.device)
    part_counts = torch.empty_like(whole_counts)

    def ranged(lo, hi, out):
        _lib.check(L.kge_rank_candidates_range(ctypes.byref(con._desc), _lib.table_ptrs([ent[lo:].data_ptr(), rel.data_ptr()]), lo, hi - lo,
                                               query.data_ptr(), ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n, None, 0, None, 0,
                                               C, flags, seed, out.data_ptr(), st), L)
    arms = {"whole": lambda: rank_eval.rank_candidates_device(con, ids, None, None, C, flags, seed, into=whole_counts),
            "range": lambda: ranged(0, chunk, part_counts)}
    times = {k: [] for k in arms}
    for fn in arms.values():
        fn()
    for _ in range(rounds):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    total = torch.zeros_like(whole_counts)
    for g in range(W):
        ranged(min(g * chunk, E), min((g + 1) * chunk, E), part_counts)
        total += part_counts
    line = {"shape": "large", "model": "TransE", "dim": D, "entities": E, "triples": n, "candidates": C, "sides": 2, "range_cut": W,
            "range_rows": chunk, "table_bytes": float(E) * D * 4, "whole": summary(times["whole"]), "range": summary(times["range"])}
    line["range_over_whole"] = round(float(np.median(times["range"]) / np.median(times["whole"])), 4)
    line["counts_sum_equal_whole"] = bool(torch.equal(total, whole_counts))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="?", default="fb", choices=("fb", "large"))
    ap.add_argument("model", nargs="?", default="TransE")
    ap.add_argument("dim", nargs="?", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_candidates.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--candidates", type=int, default=0)
    ap.add_argument("--entities", type=int, default=5000000)
    ap.add_argument("--triples", type=int, default=100000)
    ap.add_argument("--range-cut", type=int, nargs="+", default=[], metavar="W")
    a = ap.parse_args()
    if a.range_cut and (a.shape != "large" or a.model != "TransE" or min(a.range_cut) < 1):
        sys.exit("--range-cut W needs the large shape, TransE and W >= 1")
    import torch
    import openkeonspark_amd as pkg
    C = a.candidates or (1000 if a.shape == "fb" else 500)
    con, tt = fb_engine(pkg, a.model, a.dim) if a.shape == "fb" else large_engine(pkg, a.model, a.dim, a.entities, a.triples)
    torch.cuda.synchronize()
    if a.range_cut:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        ok = True
        for W in a.range_cut:
            line = range_cut(con, tt, C, W, a.rounds)
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            ok = ok and line["counts_sum_equal_whole"]
        if not ok:
            sys.exit("the ranges' counts do not sum to the whole table's")
        return
    h, t, r = tt[:, 0], tt[:, 1], tt[:, 2]
    full = a.shape == "fb"

    def form(fused):
        con.lib.kge_set_option(b"rankc_fused", fused)
        try:
            return con.rank_triples_sampled(h, t, r, C, seed=1)[0]
        finally:
            con.lib.kge_set_option(b"rankc_fused", 1)

    arms = {"fused": lambda: form(1), "two_stage": lambda: form(0)}
    if full:
        arms["rank_triples"] = lambda: con.rank_triples(h, t, r)[0]
    times, last = {k: [] for k in arms}, {}
    for k, fn in arms.items():                  # warm-up: the filter upload and every workspace
        fn()
    for _ in range(a.rounds):                   # interleaved rounds
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    D = con.hidden_size if a.model != "TransR" else con.rel_size
    gathered = float(len(h)) * 2 * C * D * 4
    line = {"shape": a.shape, "model": a.model, "dim": a.dim, "entities": con.entTotal, "triples": int(len(h)), "candidates": C, "sides": 2,
            "table_bytes": float(con.entTotal) * D * 4, "gathered_bytes": gathered}
    for k in arms:
        line[k] = summary(times[k])
    for k in ("fused", "two_stage"):
        line[k + "_gather_TBps"] = round(gathered / float(np.median(times[k])) / 1e12, 4)
    line["fused_over_two_stage"] = round(float(np.median(times["fused"]) / np.median(times["two_stage"])), 4)
    line["counts_equal_two_stage"] = bool(np.array_equal(last["fused"], last["two_stage"]))
    line["MRR_filter_tail_sampled"] = float((1.0 / (1 + last["fused"][:, 0, 1])).mean())
    if full:
        line["MRR_filter_tail_full"] = float((1.0 / (1 + last["rank_triples"][:, 0, 1])).mean())
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    if not line["counts_equal_two_stage"]:
        sys.exit("the fused kernel's counts differ from the two-stage form's")


if __name__ == "__main__":
    main()
