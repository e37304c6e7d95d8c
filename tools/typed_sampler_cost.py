#!/usr/bin/env python3
"""What type-constrained negative sampling (Config.set_type_constrained_sampling) costs on the FB15k-237-shaped typed graph
(synthetic.FB15K237_TYPED) at the benchmark's TransE configuration (D = 200, 25 negatives, nbatches 8, Adam, Bernoulli):
  index   -- host build of the typed index: wall time of kge_set_typed_sampling(1) after the type file is imported
             (median of --builds; every build starts from a stale index, as after importTypeFiles)
  sampler -- the sampler kernel on its own, untyped and typed, same batch shape and stream states: mean of the engine's event
             pairs around its launches (option time_sampler, kge_kernel_ms_mean("sampler"))
  step    -- train_step per step (host clock around --steps synchronised at the ends), untyped with the sampler riding in the
             step's launches (the default), untyped with the sampler launched on its own (ride_shares = 0: what the typed mode
             does, without its picks), and typed; --runs of each, interleaved
One JSON line; --out appends it to a file.
usage: typed_sampler_cost.py [--steps 200] [--warmup 20] [--runs 3] [--builds 5] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

DIM, NEG, NBATCHES, W = 200, 25, 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from openkeonspark_amd import Config, TransE, _lib
    from openkeonspark_amd.synthetic import make_typed_dataset, FB15K237_TYPED
    tmp = tempfile.TemporaryDirectory(prefix="okes_typed_")
    path = make_typed_dataset(os.path.join(tmp.name, "fb15k237_typed"), FB15K237_TYPED)

    def config(typed):
        con = Config()
        con.set_in_path(path); con.set_work_threads(W); con.set_bern(1); con.set_dimension(DIM); con.set_nbatches(NBATCHES)
        con.set_ent_neg_rate(NEG); con.set_margin(1.0); con.set_alpha(0.001); con.set_opt_method("Adam")
        con.set_type_constrained_sampling(typed)
        con.init()
        con.set_model_and_session(TransE)
        return con

    L = _lib.lib()
    res = dict(tool="typed_sampler_cost", dim=DIM, neg=NEG, steps=args.steps)

    # ---- host index build ----
    con = config(False)
    res.update(entities=con.entTotal, relations=con.relTotal, train=con.trainTotal, batch=con.batch_size)
    builds = []
    for _ in range(args.builds):
        L.kge_clear_error()
        L.importTypeFiles()                      # marks the typed index stale
        _lib.raise_if_error(L)
        t0 = time.perf_counter()
        _lib.check(L.kge_set_typed_sampling(1), L)
        builds.append((time.perf_counter() - t0) * 1e3)
        L.kge_set_typed_sampling(0)
    res["index_build_ms"] = round(statistics.median(builds), 3)
    res["index_build_ms_all"] = [round(x, 3) for x in builds]

    # ---- the sampler kernel alone ----
    B, slots = con.batch_size, 1 + NEG
    buf = torch.zeros((3, B * slots), dtype=torch.int32, device="cuda")
    seeds = np.ascontiguousarray(con.get_stream_states(), dtype=np.uint64)

    def sampler_ms(typed):
        _lib.check(L.kge_set_typed_sampling(1 if typed else 0), L)
        L.kge_set_stream_states(seeds.ctypes.data, W)
        nl = ctypes.c_int64()
        for i in range(args.warmup + args.steps):
            if i == args.warmup:
                torch.cuda.synchronize()
                L.kge_set_option(b"time_sampler", 1)
            _lib.check(L.kge_sampling_device(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), B, NEG, 0, 0, W, B,
                                             ctypes.byref(nl), None), L)
        torch.cuda.synchronize()
        ms, n = ctypes.c_float(), ctypes.c_int64()
        _lib.check(L.kge_kernel_ms_mean(b"sampler", ctypes.byref(ms), ctypes.byref(n)), L)
        L.kge_set_option(b"time_sampler", 0)
        return ms.value * 1e3

    samp = {"untyped": [], "typed": []}
    for _ in range(args.runs):
        samp["untyped"].append(round(sampler_ms(False), 2))
        samp["typed"].append(round(sampler_ms(True), 2))
    L.kge_set_typed_sampling(0)
    res["sampler_us"] = {k: statistics.median(v) for k, v in samp.items()}
    res["sampler_us_all"] = samp

    # ---- the training step ----
    def step_us(con):
        for _ in range(args.warmup):
            con.train_step(sync=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            con.train_step(sync=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e6

    default_shares = -1      # automatic (include/kge_mi355.h "ride_shares")
    steps = {"untyped": [], "untyped_own_launch": [], "typed": []}
    for _ in range(args.runs):
        for kind in steps:
            L.kge_set_option(b"ride_shares", 0 if kind == "untyped_own_launch" else default_shares)
            c = config(kind == "typed")
            steps[kind].append(round(step_us(c), 2))
            del c
    L.kge_set_option(b"ride_shares", default_shares)
    L.kge_set_typed_sampling(0)
    res["step_us"] = {k: statistics.median(v) for k, v in steps.items()}
    res["step_us_all"] = steps
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
