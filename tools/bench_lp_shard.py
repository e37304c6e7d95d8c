#!/usr/bin/env python3
"""Link prediction over a row range of the entity table (kge_link_prediction_range + kge_link_prediction_finish, the ranker
of a table sharded across ranks): one JSON line per workload, a host clock around synchronised calls after a warm-up.
  (a) the FB15k-237-shaped test set (synthetic.FB15K237_TYPED: 14 541 entities, 20 466 test triples x 2 sides, TransE D = 200)
      as one range, against kge_link_prediction on the same table;
  (b) one rank's share of BASELINE config #5 in one process: 6.25 M rows x D 512 as one range, 4 096 test triples x 2 sides
      (a synthetic graph with 6.25 M entities; the table scaled so that scores spread as a trained one's would not).
Floors as DESIGN 4.9.1 computes them: max(candidate bytes / 8 TB/s, lane ops / 78.6 T lane-ops/s), lane ops = candidates x
requests x D x 2 (one fma and one add of |.| per element).
Kernel times: run under `rocprofv3 --kernel-trace --stats` (lp_range_kernel, lp_finish_kernel; rank_kernel / lp_score_kernel
for kge_link_prediction).
usage: bench_lp_shard.py [--which a,b] [--reps R] [--dir DIR]"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

LANE_OPS = 256 * 4 * 32 * 2.4e9   # CUs x SIMDs x lanes x clock: 78.6 T lane-ops/s
HBM = 8e12


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def floor_ms(rows, requests, D):
    return max(rows * D * 4 / HBM, rows * requests * D * 2 / LANE_OPS) * 1e3


def range_call(con, count):
    """A closure running the new entry points over the whole table as one range, test triples [0, count), both sides."""
    import torch
    from openkeonspark_amd import _lib
    L, st = con.lib, con._stream()
    E = con.entTotal
    ids = torch.empty(2 * count, dtype=torch.int32, device=con.device)
    _lib.check(L.kge_test_entity_ids(0, count, ids.data_ptr(), st), L)
    query = con._tables[0].index_select(0, ids.long()).contiguous()
    counts = torch.empty((count, 2, 4), dtype=torch.int64, device=con.device)
    keys = torch.empty_like(counts)
    out = np.zeros((count, 2, 8), dtype=np.int64)

    def run():
        _lib.check(L.kge_link_prediction_range(ctypes.byref(con._desc), con._tab_ptrs, 0, E, query.data_ptr(), 0, count, 1,
                                               counts.data_ptr(), keys.data_ptr(), st), L)
        _lib.check(L.kge_link_prediction_finish(0, count, 1, counts.data_ptr(), keys.data_ptr(), out.ctypes.data, st), L)
        return out
    return run


def make_config(d, dim, scale):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(d); con.set_work_threads(8); con.set_dimension(dim)
    con.set_test_link_prediction(True)
    con.init()
    con.set_model_and_session(pkg.TransE)
    for t in con._tables:
        t.mul_(scale)
    con.tables_changed()
    return con


def workload_a(d, reps):
    con = make_config(d, 200, 3.0)
    n = int(con.lib.getTestTotal())
    run = range_call(con, n)
    new = run()
    old, _ = con.link_prediction()
    t_new = timed(run, reps)
    t_old = timed(lambda: con.link_prediction(), reps)
    E = con.entTotal
    return dict(workload="a_fb15k237_one_range", E=int(E), D=200, triples=n, requests=2 * n, range_ms=t_new * 1e3,
                link_prediction_ms=t_old * 1e3, speedup=t_old / t_new, floor_ms=floor_ms(E, 2 * n, 200),
                x_floor=t_new * 1e3 / floor_ms(E, 2 * n, 200), counts_equal_fraction=float((new[:, :, :4] == old[:, :, :4]).mean()))


def workload_b(d, reps):
    con = make_config(d, 512, 1.0)
    n = 4096
    run = range_call(con, n)
    run()
    t = timed(run, reps)
    E = con.entTotal
    return dict(workload="b_config5_one_rank_share", rows=int(E), D=512, triples=n, requests=2 * n, range_ms=t * 1e3,
                floor_ms=floor_ms(E, 2 * n, 512), x_floor=t * 1e3 / floor_ms(E, 2 * n, 512))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="a,b")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the synthetic graphs are written (default: a private temp dir, removed)")
    args = ap.parse_args()
    from openkeonspark_amd import synthetic
    base = args.dir or tempfile.mkdtemp(prefix="bench_lp_shard_")
    try:
        for w in args.which.split(","):
            if w == "a":
                d = synthetic.make_typed_dataset(os.path.join(base, "fb15k237_typed"), synthetic.FB15K237_TYPED)
                print(json.dumps(workload_a(d, args.reps)), flush=True)
            elif w == "b":
                d = synthetic.make_typed_dataset(os.path.join(base, "config5_rank_share"), synthetic.FB15K237_TYPED,
                                                 entities=6_250_000, train=200_000, valid=1_000, test=4_096, seed=5)
                print(json.dumps(workload_b(d, args.reps)), flush=True)
    finally:
        if args.dir is None:
            shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
