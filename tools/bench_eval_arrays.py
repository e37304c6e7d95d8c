#!/usr/bin/env python3
"""Evaluation import time on one synthetic graph: the file path (importTestFiles, then the two further host sorts and the uploads
of the first device use -- code this change leaves as it was) against init_evaluation_from_arrays(..., derive_types=True) plus
first use with the host build and with the device build (csrc/eval_build.hip).  Wall clock around a synchronised call, the
median of RUNS fresh processes each; the training import is outside the timed region.  Prints one JSON line.
usage: bench_eval_arrays.py [UNION_TRIPLES=4194304] [ENTITIES=1000000] [RELATIONS=1000] [RUNS=5]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def first_use(con):
    """What the first ranking call pays: the evaluation arrays on the device (a 16-byte read back of the (t,r,h) order)."""
    import torch
    buf = np.zeros(4, np.int32)
    assert con.lib.kge_eval_copy(b"all_t", buf.ctypes.data, 16) > 0
    torch.cuda.synchronize()


def child(variant, d):
    import torch
    from openkeonspark_amd import _lib
    from openkeonspark_amd.Config import Config
    torch.cuda.init()
    con = Config()
    con.set_work_threads(8)
    if variant == "files":
        con.set_in_path(d)
        con.init()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        con.init_link_prediction()
        first_use(con)
    else:
        z = np.load(os.path.join(d, "arrays.npz"))
        _lib.check(con.lib.kge_set_option(b"eval_index_device_min", 0 if variant == "arrays_device" else -1), con.lib)
        con.init_from_arrays(int(z["E"]), int(z["R"]), z["h"], z["t"], z["r"])
        valid, test = tuple(z["valid"]), tuple(z["test"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        con.init_evaluation_from_arrays(valid, test, derive_types=True)
        first_use(con)
    print("SECONDS %.6f" % (time.perf_counter() - t0), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    total = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 22
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    R = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    from openkeonspark_amd.synthetic import generate_triples, write_openke_dir
    n_eval = max(total // 80, 1)
    n_tr = total - 2 * n_eval
    h, t, r = generate_triples(E, R, total, 22)
    out = {"union_triples": total, "entities": E, "relations": R, "valid": n_eval, "test": n_eval, "runs": runs}
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        write_openke_dir(d, E, R, h[:n_tr], t[:n_tr], r[:n_tr])
        cut = lambda lo, hi: np.stack([h[lo:hi], t[lo:hi], r[lo:hi]])
        for name, (lo, hi) in (("valid", (n_tr, n_tr + n_eval)), ("test", (n_tr + n_eval, total))):
            with open(d + name + "2id.txt", "w") as f:
                f.write("%d\n" % (hi - lo))
                np.savetxt(f, cut(lo, hi).T, fmt="%d")
        np.savez(d + "arrays.npz", E=E, R=R, h=h[:n_tr], t=t[:n_tr], r=r[:n_tr], valid=cut(n_tr, n_tr + n_eval), test=cut(n_tr + n_eval, total))
        for variant in ("files", "arrays_host", "arrays_device"):
            times = []
            for _ in range(runs):
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, d], capture_output=True, text=True,
                                     timeout=600)
                line = [l for l in res.stdout.splitlines() if l.startswith("SECONDS ")]
                if res.returncode != 0 or not line:
                    sys.exit("bench_eval_arrays: %s failed (exit %d)\n%s" % (variant, res.returncode, res.stderr[-2000:]))
                times.append(float(line[0].split()[1]))
            out[variant + "_seconds"] = round(statistics.median(times), 4)
            out[variant + "_all"] = [round(x, 4) for x in times]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
