#!/usr/bin/env python3
"""Wall time of the per-relation ROC AUC of the validation split (Config.roc_auc("valid")) on the FB15k-237-shaped typed graph
(synthetic.FB15K237_TYPED: 17 535 validation triples, 237 relations), D = 200, after --train-steps training steps so that the
score ranges are those of a run:
  host   -- what a user had before kge_tc_roc: two test_step calls (scores to the host), the library's host get_TPFP for every
            relation with validation triples (grid x scores comparisons each), the integer area in NumPy;
  device -- Config.roc_auc("valid"): getValidBatch's draw, one upload, kge_predict x 2 -> kge_tc_roc with d_tpfp = NULL, one
            [R][2] buffer read back.
roc_auc draws new negatives on every call, so each repetition times the device call first and then the host form on the batch
that call left in the Config's buffers (the host time leaves the draw out); their per-relation values must be equal at every
repetition.  The host get_TPFP counts over the library's TEST ranges, so the dataset directory carries the validation list as
its test list too.  Host clock around a synchronised call, median of --checks after --warmup.  Also: the device call by stage.
One JSON line per model; --out appends them to a file.
usage: roc_time.py [--models TransE,TransH] [--checks 20] [--warmup 3] [--train-steps 300] [--out FILE]"""
import argparse
import ctypes
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


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def host_roc(con, valid):
    """(area2, n_r) of every relation from host scores: get_TPFP gives TP(i) / FP(i) on the grid; the closing segment to
    (n_r, n_r) completes twice the trapezoid area."""
    L = con.lib
    ph, pt, pr, nh, nt, nr = valid
    pos = np.ascontiguousarray(con.test_step(ph, pt, pr).reshape(-1), dtype=np.float32)
    neg = np.ascontiguousarray(con.test_step(nh, nt, nr).reshape(-1), dtype=np.float32)
    out = np.zeros((con.relTotal, 2), np.int64)
    grids = np.zeros(con.relTotal, np.int64)
    counts = np.bincount(pr, minlength=con.relTotal)
    for r in np.nonzero(counts)[0]:
        n = L.get_n_interval(int(r), pos.ctypes.data, neg.ctypes.data)
        ptr = L.get_TPFP(int(r), pos.ctypes.data, neg.ctypes.data, pos.ctypes.data, neg.ctypes.data)
        c = np.ctypeslib.as_array(ptr, shape=(2 * (n + 1),))
        n_r = int(counts[r])
        y = np.concatenate([[0], c[:n + 1], [n_r]])
        x = np.concatenate([[0], c[n + 1:], [n_r]])
        out[r] = (int(((x[1:] - x[:-1]) * (y[1:] + y[:-1])).sum()), n_r)
        grids[r] = n + 1
    return out, grids


def run_model(d, model, args):
    import torch
    import openkeonspark_amd as pkg
    from openkeonspark_amd import _lib
    con = pkg.Config()
    con.set_in_path(d); con.set_work_threads(8); con.set_bern(0); con.set_dimension(200); con.set_nbatches(100)
    con.set_ent_neg_rate(1); con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method("SGD")
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    for _ in range(args.train_steps):
        con.train_step(sync=False)
    torch.cuda.synchronize()
    L = con.lib
    vp = ctypes.c_void_p
    L.get_n_interval.argtypes = [ctypes.c_int64, vp, vp]; L.get_n_interval.restype = ctypes.c_int64
    L.get_TPFP.argtypes = [ctypes.c_int64, vp, vp, vp, vp]; L.get_TPFP.restype = ctypes.POINTER(ctypes.c_int64)
    R = con.relTotal
    auc2 = torch.empty((R, 2), dtype=torch.int64, device=con.device)
    offsets = np.zeros(R + 1, np.int64)

    def device_roc():
        ids = con._tc_upload(valid)
        v = con._tc_scores(ids)
        _lib.check(L.kge_tc_roc(v[0].data_ptr(), v[1].data_ptr(), ids.shape[1], 0, v[0].data_ptr(), v[1].data_ptr(), ids.shape[1],
                                auc2.data_ptr(), None, 0, offsets.ctypes.data, con._stream()), L)
        return auc2.cpu().numpy()

    host_s, dev_s = [], []
    for i in range(args.warmup + args.checks):
        td, res = wall(lambda: con.roc_auc("valid"))
        valid = [con.valid_pos_h, con.valid_pos_t, con.valid_pos_r, con.valid_neg_h, con.valid_neg_t, con.valid_neg_r]
        th, (want, grids) = wall(lambda: host_roc(con, valid))
        have = want[:, 1] > 0
        assert np.array_equal(res["n"], want[:, 1]) and np.isnan(res["auc"][~have]).all()
        assert res["auc"][have].tolist() == [int(a) / (2 * int(k) * int(k)) for a, k in want[have]]
        if i >= args.warmup:
            host_s.append(th); dev_s.append(td)
    assert np.array_equal(device_roc(), want)
    stages = dict(upload=[], predict=[], roc_call_returns=[], roc_done=[], read=[])
    for i in range(args.warmup + args.checks):
        tu, ids = wall(lambda: con._tc_upload(valid))
        tp_, v = wall(lambda: con._tc_scores(ids))
        t0 = time.perf_counter()
        _lib.check(L.kge_tc_roc(v[0].data_ptr(), v[1].data_ptr(), ids.shape[1], 0, v[0].data_ptr(), v[1].data_ptr(), ids.shape[1],
                                auc2.data_ptr(), None, 0, offsets.ctypes.data, con._stream()), L)
        t1 = time.perf_counter()      # the call has made its one wait: ranges, finiteness, n_interval; the rest is enqueued
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        tr, _ = wall(lambda: auc2.cpu())
        if i >= args.warmup:
            for k, x in zip(("upload", "predict", "roc_call_returns", "roc_done", "read"), (tu, tp_, t1 - t0, t2 - t0, tr)):
                stages[k].append(x)
    n = want[:, 1]
    have = n > 0
    auc = want[have, 0] / (2.0 * n[have] * n[have])
    h, v = statistics.median(host_s), statistics.median(dev_s)
    return dict(model=model, D=200, valid=len(valid[0]), R=int(R), train_steps=args.train_steps, checks=args.checks,
                relations_with_auc=int(have.sum()), auc_macro=float(auc.mean()), auc_weighted=float((n[have] * auc).sum() / n[have].sum()),
                grid_points_total=int(grids.sum()), grid_points_max=int(grids.max()),
                host_ms=h * 1e3, host_ms_min_max=[min(host_s) * 1e3, max(host_s) * 1e3],
                device_ms=v * 1e3, device_ms_min_max=[min(dev_s) * 1e3, max(dev_s) * 1e3],
                device_stage_ms={k: statistics.median(x) * 1e3 for k, x in stages.items()}, host_over_device=h / v)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="TransE,TransH")
    p.add_argument("--checks", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--train-steps", type=int, default=300)
    p.add_argument("--out", default="")
    args = p.parse_args()
    from openkeonspark_amd.synthetic import make_typed_dataset, FB15K237_TYPED
    d = tempfile.mkdtemp(prefix="okes_roc_") + "/"
    try:
        make_typed_dataset(d, FB15K237_TYPED)
        shutil.copyfile(os.path.join(d, "valid2id.txt"), os.path.join(d, "test2id.txt"))      # host get_TPFP reads the test ranges
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
