"""CPU search for the initialisation seeds of tests/test_gpu_shared_in_chunk_step.py (no GPU: run it anywhere the package builds).

A run of that test is replayed on the host: the positives of every step come from the CPU oracle's sampler (the device sampler's
bit-exact twin, started from the engine's stream states), the lists from tests/shared_in_chunk_ref.py host_lists, the tables from
the models' own host initialisation, and the steps from reference_step (fp64 gradients through the fp32 optimizer rules).  For
each run the seeds 1, 2, ... are tried and the near-zero elements (|e| < 1e-6 in any scored triple) and the smallest distance of
a hinge from its kink are printed per seed; the first seed with none of the former and no hinge within 1e-5 is kept.

    python tools/shared_in_chunk_seeds.py [--tries 8]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tries", type=int, default=8)
    args = ap.parse_args()
    import openkeonspark_amd as ok
    import shared_in_chunk_ref as icref
    from oracle import oracle
    from test_gpu_shared_step import ADAM_EPS, E, MARGIN, N, P, R, SEED, graph
    from test_gpu_shared_in_chunk_step import K, RATES
    models = {"transe": ok.TransE, "transh": ok.TransH, "transd": ok.TransD, "transr": ok.TransR}
    h, t, r = graph()
    train = set(zip(h.tolist(), t.tolist(), r.tolist()))
    derived = icref.derived_type_lists(h, t, r, R)

    def replay(model, opt, typed, D, steps, seed):
        con = ok.Config()
        con.set_work_threads(4); con.set_bern(1); con.set_dimension(D); con.set_ent_neg_rate(N); con.set_rel_neg_rate(0)
        con.set_nbatches(10); con.set_margin(MARGIN)
        con.seed, con.device = seed, "cpu"
        con.lib.kge_set_option(b"libc_rand_restart", 1)
        con.init_from_arrays(E, R, h, t, r)
        bern = np.zeros(R, np.float32)
        assert con.lib.kge_index_copy(b"bern_prob", bern.ctypes.data, bern.nbytes) == bern.nbytes
        kg = oracle.KG(arrays=(E, R, h, t, r, 0), work_threads=4, bern=1)
        kg.set_stream_states(con.get_stream_states())
        m = models[model](config=con, define=True)
        s = {name: m.parameter_lists[name].numpy().copy() for name in icref.TABLES[model]}
        for i, name in enumerate(icref.TABLES[model]):
            if opt == "LazyAdam":
                s["m%d" % i], s["v%d" % i] = np.zeros_like(s[name]), np.zeros_like(s[name])
            if opt == "Adagrad":
                s["a%d" % i] = np.full_like(s[name], con.adagrad_initial_accumulator)
        B = con.batch_size
        near, kink = 0, np.inf
        for step in range(steps):
            ph, pt, pr, _ = kg.sampling(B, 0, 0)
            h2, t2, r2, cand, pair, perm, chunks = icref.host_lists(ph, pt, pr, P, E, R, N, K, SEED, step, train, bern, derived if typed else None)
            lr_t = oracle.adam_lr_t(RATES[model, opt], con.adam_beta1, con.adam_beta2, step + 1) if opt == "LazyAdam" else 0.0
            w = icref.reference_step(model, opt, s, (h2, t2, r2, cand, pair, chunks), lr_t, RATES[model, opt], E, R, MARGIN, ADAM_EPS)
            near += w["near"]; kink = min(kink, w["min_kink"])
            s.update(w["state"])
        return near, kink

    runs = [("transe", opt, typed, 32, 3) for opt in ("SGD", "LazyAdam", "Adagrad") for typed in (False, True)]
    runs += [("transe", "SGD", True, 50, 1), ("transh", "SGD", False, 32, 3), ("transd", "SGD", False, 32, 3), ("transr", "SGD", False, 32, 1)]
    for model, opt, typed, D, steps in runs:
        tried = []
        for seed in range(1, args.tries + 1):
            near, kink = replay(model, opt, typed, D, steps, seed)
            tried.append("%d: %d%s" % (seed, near, "" if kink >= 1e-5 else " (kink %.1e)" % kink))
            if near == 0 and kink >= 1e-5:
                break
        print("%s %s typed %d width %d, %d steps -> %s" % (model, opt, typed, D, steps, ", ".join(tried)), flush=True)


if __name__ == "__main__":
    main()
