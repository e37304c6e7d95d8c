#!/usr/bin/env python3
"""Top-k entity prediction over a row range of the entity table (kge_topk_entities_range + kge_topk_merge_keys, the path of
Config.top_k_tails / top_k_heads on a table sharded across ranks): one JSON line per workload, a host clock around
synchronised calls after a warm-up, against kge_topk_entities on the same queries (the results are checked bit for bit).
  (a) FB15k-237 shape (synthetic.FB15K237_TYPED: 14 541 entities, TransE D = 200): every test triple, both sides (2 x 20 466
      queries), k = 10, filtered, the whole table as one range + the merge;
  (b) one rank's share of BASELINE config #5: 6.25 M rows x D 512, n = 16 and 256 tail queries, k = 10, on the fly (random
      rows), as one range + the merge -- against kge_topk_entities on the same 6.25 M-row table and DESIGN 4.9.1's floor
      max(candidate bytes / 8 TB/s, lane ops / 78.6 T lane-ops/s).
The exchange between ranks is not timed here (gloo / RCCL, the caller's network).
Kernel times: run under `rocprofv3 --kernel-trace --stats` (topk_select_kernel / topk_merge_kernel / topk_table_kernel).
usage: bench_topk_shard.py [--which a,b] [--reps R] [--rows N] [--dir DIR]"""
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


def calls(con, fixed, rel, head, k, flags):
    """Closures: kge_topk_entities over the table, and kge_topk_entities_range over the table as one range + kge_topk_merge_keys
    (the query rows gathered once, outside the timed calls)."""
    import torch
    from openkeonspark_amd import _lib
    L, st, dev = con.lib, con._stream(), con.device
    n, E = len(fixed), con.entTotal
    f = torch.as_tensor(fixed, dtype=torch.int32, device=dev)
    r = torch.as_tensor(rel, dtype=torch.int32, device=dev)
    h = torch.as_tensor(head, dtype=torch.int32, device=dev)
    qrows = con._tables[0].index_select(0, f.long()).contiguous()
    keys = torch.empty((n, k), dtype=torch.int64, device=dev)
    out = [torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.float32, device=dev)]
    ref = [torch.empty_like(out[0]), torch.empty_like(out[1])]

    def whole():
        _lib.check(L.kge_topk_entities(ctypes.byref(con._desc), con._tab_ptrs, f.data_ptr(), r.data_ptr(), h.data_ptr(), n, k, flags,
                                       ref[0].data_ptr(), ref[1].data_ptr(), st), L)

    def ranged():
        _lib.check(L.kge_topk_entities_range(ctypes.byref(con._desc), con._tab_ptrs, 0, E, qrows.data_ptr(), f.data_ptr(), r.data_ptr(),
                                             h.data_ptr(), n, k, flags, keys.data_ptr(), st), L)
        _lib.check(L.kge_topk_merge_keys(keys.data_ptr(), n, 1, k, out[0].data_ptr(), out[1].data_ptr(), st), L)

    def same_bits():
        whole(); ranged()
        return bool(torch.equal(out[0], ref[0]) and torch.equal(out[1].view(torch.int32), ref[1].view(torch.int32)))
    return whole, ranged, same_bits


def workload_a(d, reps):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(d); con.set_work_threads(8); con.set_dimension(200)
    con.set_test_link_prediction(True)
    con.init()
    con.set_model_and_session(pkg.TransE)
    for t in con._tables:      # spread the scores as a trained table's would
        t.mul_(3.0)
    con.tables_changed()
    tr = np.loadtxt(os.path.join(d, "test2id.txt"), dtype=np.int64, skiprows=1, ndmin=2)
    n = len(tr)
    fixed = np.concatenate([tr[:, 0], tr[:, 1]])
    rel = np.concatenate([tr[:, 2], tr[:, 2]])
    head = np.concatenate([np.zeros(n), np.ones(n)]).astype(np.int32)
    whole, ranged, same = calls(con, fixed, rel, head, 10, 1)
    ok = same()
    t_whole, t_range = timed(whole, reps), timed(ranged, reps)
    return dict(workload="a_fb15k237_one_range", E=int(con.entTotal), D=200, queries=2 * n, k=10, filtered=True,
                range_merge_ms=round(t_range * 1e3, 3), topk_entities_ms=round(t_whole * 1e3, 3),
                ratio=round(t_range / t_whole, 3), bits_equal=ok)


def workload_b(rows, reps):
    import openkeonspark_amd as pkg
    D, R = 512, 16
    rng = np.random.default_rng(5)
    nt = 4096
    con = pkg.Config()
    con.set_work_threads(8); con.set_dimension(D); con.set_nbatches(1)
    con.init_from_arrays(rows, R, rng.integers(0, rows, nt), rng.integers(0, rows, nt), rng.integers(0, R, nt))
    con.set_model_and_session(pkg.TransE)
    con.lib.kge_set_option(b"topk_table_max_bytes", 0)
    res = dict(workload="b_config5_one_rank_share", rows=rows, D=D, k=10, on_the_fly=True, per_n={})
    q_per_block = 8   # topk.hip: queries per workgroup at D <= 512
    try:
        for n in (16, 256):
            fixed = rng.integers(0, rows, n)
            rel = rng.integers(0, R, n)
            whole, ranged, same = calls(con, fixed, rel, np.zeros(n, dtype=np.int32), 10, 0)
            ok = same()
            t_whole, t_range = timed(whole, reps), timed(ranged, reps)
            blocks = (n + q_per_block - 1) // q_per_block
            bytes_read = rows * D * 4 * blocks
            lane_ops = rows * blocks * (3 * D + 64 * 7) + rows * n * (2 * D + 64 * 7)
            floor = max(bytes_read / HBM, lane_ops / LANE_OPS)
            res["per_n"][str(n)] = dict(range_merge_ms=round(t_range * 1e3, 3), topk_entities_ms=round(t_whole * 1e3, 3),
                                        ratio=round(t_range / t_whole, 3), floor_ms=round(floor * 1e3, 3),
                                        x_floor=round(t_range / floor, 2), bits_equal=ok)
    finally:
        con.lib.kge_set_option(b"topk_table_max_bytes", 1 << 30)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=6_250_000)
    ap.add_argument("--dir", default=None, help="where the synthetic graph of (a) is written (default: a private temp dir, removed)")
    args = ap.parse_args()
    from openkeonspark_amd import synthetic
    base = args.dir or tempfile.mkdtemp(prefix="bench_topk_shard_")
    try:
        for w in args.which.split(","):
            if w == "a":
                d = synthetic.make_typed_dataset(os.path.join(base, "fb15k237_typed"), synthetic.FB15K237_TYPED)
                print(json.dumps(workload_a(d, args.reps)), flush=True)
            elif w == "b":
                print(json.dumps(workload_b(args.rows, args.reps)), flush=True)
    finally:
        if args.dir is None:
            shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
