#!/usr/bin/env python3
"""Relation prediction (Config.relation_prediction / top_k_relations, kge_relation_prediction / kge_topk_relations): one JSON
line per model on the FB15k-237-shaped typed graph (synthetic.FB15K237_TYPED: valid / test / type files), D = 200 (TransR
200 x 200), with a host clock around synchronised calls after a warm-up:
  relation_prediction over the whole test set (20 466 triples, all four counts), top_k_relations(k=10, filtered=True) over
  the same (h, t) pairs, and the predict_relation loop (200 queries, extrapolated to the test set);
plus the floors computed from the shapes: lane ops / 78.6 T lane-ops/s for the vector models, and for TransR the FLOPs of
projecting every distinct test entity by every relation matrix at 157.3 TFLOP/s fp32 (and the kernel's share of that peak
when --kernel-ms gives the projection kernel's time from a trace).
Kernel times: run under `rocprofv3 --kernel-trace --stats` (relpred_score_kernel, relpred_project_kernel, relpred_norm_kernel,
relpred_score_transr_kernel, relpred_topk_kernel, relpred_rank_kernel).
usage: bench_relpred.py [--models TransE,TransH,TransD,TransR] [--reps R] [--loop N]"""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

LANE_OPS = 256 * 4 * 32 * 2.4e9   # CUs x SIMDs x lanes x clock: 78.6 T lane-FMA/s
FP32_FLOPS = 157.3e12


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def floors(model, n, R, D, distinct):
    pairs = n * R
    if model == "TransR":
        flops = distinct * R * D * D * 2
        return dict(flops=flops, floor_ms=flops / FP32_FLOPS * 1e3, per_slot_flops=2 * n * R * D * D * 2)
    ops_per_elem = 3 if model == "TransE" else 9   # |h + r - t| vs. two projections + two norms + the L1 sum
    ops = pairs * D * ops_per_elem
    return dict(lane_ops=ops, floor_ms=ops / LANE_OPS * 1e3)


def run_model(d, model, reps, loop_n):
    import torch
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(d); con.set_work_threads(8); con.set_dimension(200)
    con.set_test_relation_prediction(True)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    total = con.lib.getTestTotal()
    a = np.loadtxt(os.path.join(d, "test2id.txt"), dtype=np.int64, skiprows=1)
    h, t = a[:, 0], a[:, 1]
    hd = torch.as_tensor(h, device=con.device)
    td = torch.as_tensor(t, device=con.device)
    rp = timed(lambda: con.relation_prediction(), reps)
    tk = timed(lambda: con.top_k_relations(hd, td, 10, filtered=True), reps)
    with contextlib.redirect_stdout(io.StringIO()):   # predict_relation prints its answer
        con.predict_relation(int(h[0]), int(t[0]), 10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(loop_n):
            con.predict_relation(int(h[i]), int(t[i]), 10)
        loop = (time.perf_counter() - t0) / loop_n * total
    distinct = len(np.unique(np.concatenate([h, t])))
    res = dict(model=model, n=int(total), R=int(con.relTotal), D=200, distinct_entities=distinct,
               relation_prediction_ms=rp * 1e3, top_k_relations_ms=tk * 1e3, predict_relation_loop_ms_extrapolated=loop * 1e3,
               speedup_vs_loop=loop / rp)
    res.update(floors(model, total, con.relTotal, 200, distinct))
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="TransE,TransH,TransD,TransR")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--loop", type=int, default=200)
    p.add_argument("--kernel-ms", type=float, default=0.0, help="TransR projection kernel time (ms) from a trace: prints its share of the fp32 peak")
    args = p.parse_args()
    from openkeonspark_amd.synthetic import make_typed_dataset, FB15K237_TYPED
    d = tempfile.mkdtemp(prefix="okes_relpred_") + "/"
    try:
        make_typed_dataset(d, FB15K237_TYPED)
        for model in args.models.split(","):
            res = run_model(d, model, args.reps, args.loop)
            if model == "TransR" and args.kernel_ms > 0:
                res["projection_share_of_fp32_peak"] = res["flops"] / (args.kernel_ms * 1e-3) / FP32_FLOPS
            print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
