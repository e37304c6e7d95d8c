#!/usr/bin/env python3
"""Wall time of one early-stop check (validation accuracy: thresholds fitted on the validation scores, then the share of
the 2 V answers they get right) on the FB15k-237-shaped typed graph (synthetic.FB15K237_TYPED: 17 535 validation triples, 237
relations), D = 200, after --train-steps training steps so that the score ranges are those of a run:
  host   -- the check as it stood before the device path: two test_step calls (scores to the host), getBestThreshold's
            grid search on one host core, NumPy counts;
  device -- Config.validation_accuracy: kge_predict x 2 -> kge_tc_fit -> kge_tc_apply, four counts read back.
The two are timed alternately, host clock around a synchronised call, median of --checks after --warmup; their values must be
equal.  Also timed: one epoch of training at that shape (nbatches steps enqueued, one synchronise), for the check's cost
relative to the epoch it interrupts.  One JSON line per model; --out appends them to a file.
usage: tclass_time.py [--models TransE,TransH] [--checks 20] [--warmup 3] [--train-steps 300] [--out FILE]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def host_check(con, valid):
    ph, pt, pr, nh, nt, nr = valid
    pos = np.ascontiguousarray(con.test_step(ph, pt, pr).reshape(-1), dtype=np.float32)
    neg = np.ascontiguousarray(con.test_step(nh, nt, nr).reshape(-1), dtype=np.float32)
    thresh = np.zeros(con.relTotal, np.float32)
    con.lib.getBestThreshold(thresh.ctypes.data, pos.ctypes.data, neg.ctypes.data)
    correct = (pos <= thresh[pr]).sum() + (neg > thresh[nr]).sum()
    return float(correct) / (2.0 * max(len(pos), 1)), pos, neg


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def run_model(d, model, args):
    import ctypes
    import torch
    import openkeonspark_amd as pkg
    import openkeonspark_amd.distribute_training as dt
    con = pkg.Config()
    con.set_in_path(d); con.set_work_threads(8); con.set_bern(0); con.set_dimension(200); con.set_nbatches(100)
    con.set_ent_neg_rate(1); con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method("SGD")
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    for _ in range(args.train_steps):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    valid = dt._init_validation(con, None)
    L = con.lib
    L.get_n_interval.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.get_n_interval.restype = ctypes.c_int64
    host_s, dev_s = [], []
    for i in range(args.warmup + args.checks):
        th, (want, pos, neg) = wall(lambda: host_check(con, valid))
        td, got = wall(lambda: con.validation_accuracy(valid))
        assert got == want, (got, want)
        if i >= args.warmup:
            host_s.append(th); dev_s.append(td)
    # the device check by stage (host clock, synchronised after each stage; the whole check above has one wait and one read)
    from openkeonspark_amd import _lib
    ids = con._tc_valid_dev[1]
    buf, counts, thresh = con._tc_result_buffer()
    stages = dict(predict=[], fit_call_returns=[], fit_done=[], apply_and_read=[])
    for i in range(args.warmup + args.checks):
        tp_, v = wall(lambda: con._tc_scores(ids))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(L.kge_tc_fit(v[0].data_ptr(), v[1].data_ptr(), ids.shape[1], thresh.data_ptr(), None, con._stream()), L)
        t1 = time.perf_counter()      # the call has waited for its status word: min / max pass done, the rest enqueued
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ta, _ = wall(lambda: (_lib.check(L.kge_tc_apply(0, thresh.data_ptr(), v[0].data_ptr(), v[1].data_ptr(), ids.shape[1],
                                                        counts.data_ptr(), None, con._stream()), L), buf[:32].cpu()))
        if i >= args.warmup:
            stages["predict"].append(tp_); stages["fit_call_returns"].append(t1 - t0)
            stages["fit_done"].append(t2 - t0); stages["apply_and_read"].append(ta)
    stage_ms = {k: statistics.median(x) * 1e3 for k, x in stages.items()}
    grids = [L.get_n_interval(r, pos.ctypes.data, neg.ctypes.data) for r in range(con.relTotal)]
    epochs = []
    for _ in range(5):
        te, _ = wall(lambda: [con.train_step(sync=False) for _ in range(con.nbatches)])
        epochs.append(te)
    h, v, e = statistics.median(host_s), statistics.median(dev_s), statistics.median(epochs[1:])
    return dict(model=model, D=200, valid=len(valid[0]), R=int(con.relTotal), train_steps=args.train_steps, checks=args.checks,
                accuracy=got, grid_points_total=int(sum(grids)) + len(grids), grid_points_max=int(max(grids)) + 1,
                host_check_ms=h * 1e3, host_check_ms_min_max=[min(host_s) * 1e3, max(host_s) * 1e3],
                device_check_ms=v * 1e3, device_check_ms_min_max=[min(dev_s) * 1e3, max(dev_s) * 1e3],
                device_stage_ms=stage_ms, host_over_device=h / v, epoch_ms=e * 1e3, epoch_steps=int(con.nbatches), batch=int(con.batch_size),
                host_check_over_epoch=h / e, device_check_over_epoch=v / e)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="TransE,TransH")
    p.add_argument("--checks", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--train-steps", type=int, default=300)
    p.add_argument("--out", default="")
    args = p.parse_args()
    from openkeonspark_amd.synthetic import make_typed_dataset, FB15K237_TYPED
    d = tempfile.mkdtemp(prefix="okes_tclass_") + "/"
    try:
        make_typed_dataset(d, FB15K237_TYPED)
        for model in args.models.split(","):
            line = json.dumps(run_model(d, model, args))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
