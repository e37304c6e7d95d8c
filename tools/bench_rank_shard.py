#!/usr/bin/env python3
"""kge_rank_triples_range (the counts-only scan of a row range for any triples) against the two paths that already rank the
same triples, in one process on the FB15k-237-shaped synthetic graph (synthetic.FB15K237_TYPED: 14 541 entities, 20 466 test
triples x 2 sides), TransE D = 200, the whole table as one range:
  range_finish  kge_link_prediction_range + kge_link_prediction_finish on the test split: the same scan with arg-min keys,
                their 64-bit atomicMin, a second kernel and the copy of [n][2][8] to the host -- the baseline;
  rank_range    kge_rank_triples_range on the same triples (h, t, r and their rows on the device), then one synchronise;
  rank_range_host  the same plus the copy of its [n][2][4] counts to the host (what range_finish's time includes);
  rank_triples  kge_rank_triples for the same triples (one host synchronisation to group by relation, its own score bits).
Method: every path is warmed up, then `--rounds` rounds alternate the paths; one sample is `--inner` calls between two device
synchronisations, host clock.  Reported per path: median, min and max of the samples in ms per call, and spread = max - min.
The baseline's spread is the run-to-run noise a difference has to exceed.  The counts of the three paths are compared on the
timed inputs (range_finish's columns 0..3 must equal rank_range's exactly).  Appends one JSON line to
profiles/rank_shard.jsonl (or --out).  Kernel times: run under `rocprofv3 --kernel-trace --stats` in a run of its own
(lp_range_kernel<true, ...> / lp_finish_kernel against lp_range_kernel<false, ...>).
usage: bench_rank_shard.py [--rounds R] [--inner K] [--dir DIR] [--out FILE]"""
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

from bench_lp_shard import floor_ms, make_config, range_call


def rank_range_call(con, count, to_host):
    """A closure running kge_rank_triples_range over the whole table as one range on test triples [0, count), both sides."""
    import torch
    from openkeonspark_amd import _lib
    L, st, E = con.lib, con._stream(), con.entTotal
    pairs = torch.empty(2 * count, dtype=torch.int32, device=con.device)
    _lib.check(L.kge_test_entity_ids(0, count, pairs.data_ptr(), st), L)
    query = con._tables[0].index_select(0, pairs.long()).contiguous()          # [count][2][D]
    ht = pairs.view(count, 2).t().contiguous()
    counts = torch.empty((count, 2, 4), dtype=torch.int64, device=con.device)

    def with_relations(rel):
        r = torch.from_numpy(np.ascontiguousarray(rel, dtype=np.int32)).to(con.device)

        def run():
            _lib.check(L.kge_rank_triples_range(ctypes.byref(con._desc), con._tab_ptrs, 0, E, query.data_ptr(), ht[0].data_ptr(),
                                                ht[1].data_ptr(), r.data_ptr(), count, 1, counts.data_ptr(), st), L)
            return counts.cpu().numpy() if to_host else counts
        return run
    return with_relations, ht


def sample(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def summary(ms):
    a = np.asarray(ms)
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), spread_ms=float(a.max() - a.min()),
                samples=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--dir", default=None, help="where the synthetic graph is written (default: a private temp dir, removed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_shard.jsonl"))
    a = ap.parse_args()
    import torch
    from openkeonspark_amd import synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_rank_shard.py measures on the GPU: no device found")
    base = a.dir or tempfile.mkdtemp(prefix="bench_rank_shard_")
    try:
        d = synthetic.make_typed_dataset(os.path.join(base, "fb15k237_typed"), synthetic.FB15K237_TYPED)
        con = make_config(d, a.dim, 3.0)
        n, E = int(con.lib.getTestTotal()), int(con.entTotal)
        baseline = range_call(con, n)
        want = baseline()[:, :, :4].copy()
        # the test split's relations in kge_link_prediction's order: test2id.txt sorted by (r, h, t)
        tok = np.loadtxt(os.path.join(d, "test2id.txt"), dtype=np.int64, skiprows=1, ndmin=2)
        tt = tok[np.lexsort((tok[:, 1], tok[:, 0], tok[:, 2]))]
        make, ht = rank_range_call(con, n, False)
        assert np.array_equal(ht.cpu().numpy().T, tt[:, :2]), "the test split's order is not (r, h, t)"
        dev_only = make(tt[:, 2])
        to_host = rank_range_call(con, n, True)[0](tt[:, 2])
        fused = lambda: con.rank_triples(tt[:, 0], tt[:, 1], tt[:, 2])
        got = to_host()
        fused_counts = fused()[0]
        paths = [("range_finish", baseline), ("rank_range", dev_only), ("rank_range_host", to_host), ("rank_triples", fused)]
        for _, fn in paths:      # warm-up: every shape of the timed window
            sample(fn, 2)
        times = {name: [] for name, _ in paths}
        for _ in range(a.rounds):
            for name, fn in paths:
                times[name].append(sample(fn, a.inner))
        res = {name: summary(ms) for name, ms in times.items()}
        floor = floor_ms(E, 2 * n, a.dim)
        line = dict(tool="bench_rank_shard", E=E, D=a.dim, triples=n, requests=2 * n, rounds=a.rounds, inner=a.inner, floor_ms=floor,
                    counts_equal_range_finish=bool(np.array_equal(got, want)),
                    counts_equal_rank_triples_fraction=float((got == fused_counts).mean()),
                    rank_range_host_minus_baseline_ms=res["rank_range_host"]["median_ms"] - res["range_finish"]["median_ms"],
                    baseline_spread_ms=res["range_finish"]["spread_ms"], **res)
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
        if not line["counts_equal_range_finish"]:
            sys.exit("kge_rank_triples_range's counts differ from kge_link_prediction_range's on the test split")
    finally:
        if a.dir is None:
            shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
