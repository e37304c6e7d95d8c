"""CPU search for the lattice seeds of tests/test_gpu_bf16_shared_step.py (no GPU: run it anywhere the package builds).

A run of that test is replayed on the host: the positives of every step come from the CPU oracle's sampler (the device sampler's
bit-exact twin, started from the engine's stream states), the lists, the fp64 forward, the exact counts and the fp64 update from the
test's own host_step, and the stored rows from tests/bf16_ref.py round_rows.  (The device forms y in fp32, so about one stored
element in 4000 differs from this replay's by one bf16 ulp: far inside the lattice's gaps, which is all the conditions ask.)  For
each run the seeds 1, 2, ... are tried; the smallest distance of a hinge from its kink and the smallest |e| over the three steps
are printed, and the first seed with kink >= 5e-4 and sign >= 1e-3 -- well above what the test asserts, since one stored element
that differs moves a hinge by about 1e-4 -- is kept.

    python tools/bf16_shared_seeds.py [--tries 20]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tries", type=int, default=20)
    args = ap.parse_args()
    import openkeonspark_amd as ok
    import bf16_ref
    import shared_in_chunk_ref as icref
    import test_gpu_bf16_shared_step as T
    from oracle import oracle
    h, t, r = T.graph()
    derived = icref.derived_type_lists(h, t, r, T.R)

    def replay(D, opt, mode, seed):
        con = ok.Config()
        con.device = "cpu"
        T.configure(con, D, opt, mode)
        kg = oracle.KG(arrays=(T.E, T.R, h, t, r, 0), work_threads=4, bern=0)
        kg.set_stream_states(con.get_stream_states())
        ent, rel = T.lattice(D, seed)
        full = np.concatenate([bf16_ref.to_bf16(ent), bf16_ref.to_bf16(rel)])
        acc = np.full(T.E + T.R, con.adagrad_initial_accumulator, np.float32) if opt == "RowAdagrad" else None
        kink = sign = np.inf
        for step in range(3):
            ph, pt, pr, _ = kg.sampling(T.B, 0, 0)
            w = T.host_step(full, acc, np.stack([ph, pt, pr]), step, mode, opt, derived if mode == "typed_in_chunk" else None)
            kink, sign = min(kink, w["want"]["min_kink"]), min(sign, w["want"]["min_sign"])
            full[w["live_rows"]] = w["stored"]
            if acc is not None:
                acc[w["live_rows"]] = w["acc"].astype(np.float32)
        return kink, sign

    found = {}
    for mode in T.MODES:
        for D in (8, 200):
            for opt in ("SGD", "RowAdagrad"):
                tried = []
                for seed in range(1, args.tries + 1):
                    kink, sign = replay(D, opt, mode, seed)
                    tried.append("%d: kink %.1e sign %.1e" % (seed, kink, sign))
                    if kink >= 5e-4 and sign >= 1e-3:
                        found[(D, opt, mode)] = seed
                        break
                print("width %d %s %s -> %s" % (D, opt, mode, ", ".join(tried)), flush=True)
    print("TABLE_SEEDS = %r" % (found,))


if __name__ == "__main__":
    main()
