#!/usr/bin/env python3
"""Batched top-k entity prediction (Config.top_k_tails / top_k_heads, kge_topk_entities): one JSON line per workload.
(a) FB15k-237-shaped graph (as tools/bench_lp.py builds it, TransE D=200 trained 30 steps): every test triple, both sides,
    k=10, filtered -- against kge_link_prediction over the same triples, kge_predict into a [chunk x E] device matrix +
    torch.topk, and the per-query predict_tail_entity loop (200 queries, extrapolated).
(b) TransE D=512 over --entities random rows (default 10 M) on the on-the-fly path: ms per call for n in {1, 16, 256},
    candidate bytes read, and the floor max(bytes / 8 TB/s, lane-ops / 78.6 T lane-ops/s).
Kernel times: run under `rocprofv3 --kernel-trace --stats` (topk_select_kernel / topk_merge_kernel).
usage: bench_topk.py [--entities N] [--skip-a] [--skip-b] [--reps R]"""
import argparse
import contextlib
import ctypes
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

HBM_BPS = 8.0e12
LANE_OPS = 256 * 4 * 32 * 2.4e9   # CUs x SIMDs x lanes x clock


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def workload_a(reps):
    import torch
    import openkeonspark_amd as pkg
    from openkeonspark_amd import _lib
    from openkeonspark_amd.synthetic import FB15K237, generate_triples, write_openke_dir
    d = tempfile.mkdtemp(prefix="okes_topk_") + "/"
    try:
        spec = FB15K237
        n_test, n_valid = 20466, 17535
        h, t, r = generate_triples(spec["entities"], spec["relations"], spec["train"] + n_test + n_valid, spec["seed"])
        n = spec["train"]
        write_openke_dir(d, spec["entities"], spec["relations"], h[:n], t[:n], r[:n])
        for name, lo, hi in (("test2id.txt", n, n + n_test), ("valid2id.txt", n + n_test, n + n_test + n_valid)):
            with open(d + name, "w") as f:
                f.write("%d\n" % (hi - lo))
                np.savetxt(f, np.stack([h[lo:hi], t[lo:hi], r[lo:hi]], axis=1), fmt="%d")
        con = pkg.Config()
        con.set_in_path(d); con.set_work_threads(8); con.set_bern(1); con.set_dimension(200); con.set_nbatches(8)
        con.set_ent_neg_rate(25); con.set_alpha(0.001); con.set_opt_method("Adam")
        con.init()
        con.init_link_prediction()
        con.set_model_and_session(pkg.TransE)
        for _ in range(30):
            con.train_step(sync=False)
        torch.cuda.synchronize()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    E = con.entTotal
    th, tt, tr = h[n:n + n_test], t[n:n + n_test], r[n:n + n_test]
    dev = con.device
    dh, dt, dr = (torch.as_tensor(x, dtype=torch.int32, device=dev) for x in (th, tt, tr))
    k = 10

    def topk_both():
        con.top_k_tails(dh, dr, k, filtered=True)
        con.top_k_heads(dt, dr, k, filtered=True)
    s_topk = timed(topk_both, reps)
    s_lp = timed(lambda: con.link_prediction(test_head=True), max(1, reps // 2))
    # kge_predict on device candidate arrays for a chunk of queries, then torch.topk (unfiltered)
    chunk = 256
    ar = torch.arange(E, dtype=torch.int32, device=dev)
    out = torch.empty(chunk * E, dtype=torch.float32, device=dev)

    def compose():
        for side in (0, 1):
            for q0 in range(0, n_test, chunk):
                q1 = min(n_test, q0 + chunk)
                m = q1 - q0
                fx = (dh if side == 0 else dt)[q0:q1].repeat_interleave(E)
                cand = ar.repeat(m)
                rr = dr[q0:q1].repeat_interleave(E)
                hh, ttt = (fx, cand) if side == 0 else (cand, fx)
                _lib.check(con.lib.kge_predict(ctypes.byref(con._desc), con._tab_ptrs, hh.data_ptr(), ttt.data_ptr(), rr.data_ptr(),
                                               m * E, out.data_ptr(), con._stream()), con.lib)
                torch.topk(out[:m * E].view(m, E), k, dim=1, largest=False)
    s_compose = timed(compose, 1)
    # the per-query host path
    nq = 200
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(nq):
            con.predict_tail_entity(int(th[i]), int(tr[i]), k)
    s_loop = (time.perf_counter() - t0) / nq * 2 * n_test
    # vector-issue floor of the scoring: per (query, candidate) 2 lane-ops x D (tail) or 3 x D (head) + team_sum over 64 lanes
    D = 200
    lane_ops = n_test * E * ((2 * D + 64 * 7) + (3 * D + 64 * 7))
    print(json.dumps({"workload": "a_fb15k237_all_test_both_sides", "model": "TransE", "dim": D, "entities": E,
                      "queries": 2 * n_test, "k": k, "filtered": True,
                      "topk_s": round(s_topk, 5), "link_prediction_s": round(s_lp, 5),
                      "predict_matrix_plus_torch_topk_s": round(s_compose, 4),
                      "per_query_predict_tail_entity_s_extrapolated": round(s_loop, 2),
                      "vector_issue_floor_s": round(lane_ops / LANE_OPS, 5)}))
    sys.stdout.flush()


def workload_b(E, reps):
    import torch
    import openkeonspark_amd as pkg
    D, R = 512, 16
    rng = np.random.default_rng(1)
    nt = 4096
    con = pkg.Config()
    con.set_work_threads(8); con.set_dimension(D); con.set_nbatches(1)
    con.init_from_arrays(E, R, rng.integers(0, E, nt), rng.integers(0, E, nt), rng.integers(0, R, nt))
    con.set_model_and_session(pkg.TransE)
    con.lib.kge_set_option(b"topk_table_max_bytes", 0)
    res = {"workload": "b_transe_direct", "dim": D, "entities": E, "k": 10, "per_n": {}}
    q_per_block = 8   # topk.hip: queries per workgroup at D <= 512
    for n in (1, 16, 256):
        f = torch.as_tensor(rng.integers(0, E, n), dtype=torch.int32, device=con.device)
        r = torch.as_tensor(rng.integers(0, R, n), dtype=torch.int32, device=con.device)
        s = timed(lambda: con.top_k_tails(f, r, 10), reps)
        blocks = (n + q_per_block - 1) // q_per_block
        bytes_read = E * D * 4 * blocks
        # per candidate and query block: normalise (2 D + team_sum + D); per candidate and query: 2 D + team_sum
        lane_ops = E * blocks * (3 * D + 64 * 7) + E * n * (2 * D + 64 * 7)
        floor = max(bytes_read / HBM_BPS, lane_ops / LANE_OPS)
        res["per_n"][str(n)] = {"ms": round(s * 1e3, 3), "candidate_GBps": round(bytes_read / s / 1e9, 1),
                                "floor_ms": round(floor * 1e3, 3), "bytes_floor_ms": round(bytes_read / HBM_BPS * 1e3, 3),
                                "issue_floor_ms": round(lane_ops / LANE_OPS * 1e3, 3), "x_floor": round(s / floor, 2)}
    con.lib.kge_set_option(b"topk_table_max_bytes", 1 << 30)
    print(json.dumps(res))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    a = ap.parse_args()
    if not a.skip_a:
        workload_a(a.reps)
    if not a.skip_b:
        workload_b(a.entities, a.reps)


if __name__ == "__main__":
    main()
