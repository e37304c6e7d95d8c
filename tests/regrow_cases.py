"""The calls of tests/test_gpu_workspace_regrow.py.  The engine's device workspaces are process-global and only grow, so what a
call finds depends on the calls before it in the process.  Every case here is a pair of calls: A at a small shape and B at a
larger one (more triples or queries, a larger batch, a wider embedding), each building its own Config so that it is a pure
function of its arguments.  `python regrow_cases.py <case> <order> <out.npz>` runs the calls of `order` (e.g. ABA) in one
process and stores every call's results as "<position>/<name>" arrays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
KG = os.path.join(ROOT, "tests", "golden", "kg_small")      # 1 000 entities, 20 relations, 6 000 / 30 / 40 triples


def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


def eval_config(model, dim):
    """kg_small with its evaluation files; tables scaled so that the scores spread (as tests/test_gpu_rank.py make_config)."""
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(KG); con.set_work_threads(1); con.set_dimension(dim); con.set_test_link_prediction(True)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    for t in con._tables:
        t.mul_(3.0)
    con.tables_changed()
    return con


def split(name):
    with open(os.path.join(KG, name + "2id.txt")) as f:
        tok = f.read().split()
    n = int(tok[0])
    return np.asarray(tok[1:1 + 3 * n], dtype=np.int64).reshape(n, 3)       # (h, t, r)


def train_config(model, dim, nbatches, n, opt, **attrs):
    """kg_small, device-sampled batches of 6 000 / nbatches positives; the rng streams of a fresh process every time."""
    import openkeonspark_amd as pkg
    lib().kge_set_option(b"libc_rand_restart", 1)
    con = pkg.Config()
    for k, v in attrs.items():
        setattr(con, k, v)
    con.set_in_path(KG); con.set_work_threads(8); con.set_bern(1); con.set_dimension(dim); con.set_nbatches(nbatches)
    con.set_ent_neg_rate(n); con.set_alpha(0.01); con.set_margin(1.0); con.set_opt_method(opt)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    return con


def train_state(con, losses):
    import torch
    torch.cuda.synchronize()
    out = {"p/" + k: v.copy() for k, v in con.get_parameters().items()}
    if con._has_slots:
        for i, k in enumerate(con.trainModel.table_names):
            out["m/" + k] = con._adam_m[i].cpu().numpy()
            out["v/" + k] = con._adam_v[i].cpu().numpy()
    out["losses"] = np.asarray(losses, np.float32)
    out["streams"] = np.asarray(con.get_stream_states(), np.uint64)
    return out


# ---- the cases: name -> (A, B), each () -> {name: array} ---------------------------------------------------------------------
def rank_transr(n, dim):
    """kge_rank_triples, TransR: the request list (n + blocks), the candidate table (E x dim), the projections ((E + 1) x dim)"""
    con = eval_config("TransR", dim)
    tt = np.concatenate([split("test"), split("valid")])[:n]
    counts, _ = con.rank_triples(tt[:, 0], tt[:, 1], tt[:, 2])
    return {"counts": counts}


def relpred_transr(E, dim, n, count):
    """kge_topk_relations over a graph of E entities (the slot map, [E], is regrown and must come back all -1; the projection
    buffer follows the chunk = n queries up, and down again once it is more than twice what the call wants), then
    kge_relation_prediction over `count` test triples of kg_small at the same width."""
    import openkeonspark_amd as pkg
    R = 9
    con = pkg.Config()
    con.set_work_threads(1); con.set_dimension(dim)
    hh = np.arange(4 * E) % E
    con.init_from_arrays(E, R, hh, (hh * 7 + 1) % E, hh % R)
    con.set_model_and_session(pkg.TransR)
    for t in con._tables:
        t.mul_(3.0)
    con.tables_changed()
    rng = np.random.default_rng(E + n)
    h, t = rng.integers(0, E, n), rng.integers(0, E, n)
    h[n // 2:] = h[:n - n // 2]            # shared entities: fewer distinct ones than slots
    ids, sc = con.top_k_relations(h, t, 5)
    ids2, sc2 = con.top_k_relations(t, h, R)          # a second call on the map the first one left behind
    con = eval_config("TransR", dim)
    ranks, _ = con.relation_prediction(0, count)
    return {"ids": ids, "scores": sc, "ids2": ids2, "scores2": sc2, "ranks": ranks}


def topk_tails(n, k, dim):
    """kge_topk_entities: the partial lists (queries x slices x k), the query order (n), the inverse norms and the table"""
    con = eval_config("TransH", dim)
    rng = np.random.default_rng(n)
    ids, sc = con.top_k_tails(rng.integers(0, con.entTotal, n), rng.integers(0, con.relTotal, n), k, filtered=True)
    return {"ids": ids, "scores": sc}


def link_prediction(count):
    """kge_link_prediction with lp_v1 = 0, 1, 0: the grouped ranker sizes `scores` alone, the generic route needs `cand` beside
    it at 32 x E however large `scores` already is"""
    con = eval_config("TransD", 24)
    out = {}
    try:
        for i, v1 in enumerate((0, 1, 0)):
            lib().kge_set_option(b"lp_v1", v1)
            out["out%d" % i], _ = con.link_prediction(first=0, count=count)
    finally:
        lib().kge_set_option(b"lp_v1", 0)
    return out


def lazy_adam_transh(nbatches, dim):
    """TransH, LazyAdam on the touched rows (kge_forward_backward_adam_rows): record ids (iota), hub sums and marks"""
    con = train_config("TransH", dim, nbatches, 2, "LazyAdam")
    assert con.sparse_inplace
    return train_state(con, [con.train_step() for _ in range(3)])


def transr_groups(nbatches, dim):
    """TransR with the group layout: keys / values, tiles, bucket_rows, P and GP (slots x dim)"""
    try:
        lib().kge_set_option(b"transr_groups", 2)
        con = train_config("TransR", dim, nbatches, 3, "SGD")
        return train_state(con, [con.train_step() for _ in range(2)])
    finally:
        lib().kge_set_option(b"transr_groups", 1)


def transe_counts(nbatches, dim):
    """TransE on the fused sign-count step: records, sort buffers, pieces, row spans"""
    con = train_config("TransE", dim, nbatches, 5, "Adam", counts_min_records=0)
    assert con.use_counts and not con.sparse_rows
    return train_state(con, [con.train_step() for _ in range(3)])


def persistent(nbatches, steps):
    """train_steps(persistent=True), TransH: the two batches, the learning rates (one per step), the relation hub copies
    (6 000 / nbatches positives over 20 relations: 2 copies at 1 500, 18 at 6 000)"""
    con = train_config("TransH", 24, nbatches, 2, "SGD")
    assert con.persistent_supported()
    start = con.get_parameters()
    out = train_state(con, con.train_steps(steps, persistent=True))
    out.update({"start/" + k: v for k, v in start.items()})
    return out


CASES = {
    "rank_transr": (lambda: rank_transr(5, 8), lambda: rank_transr(70, 32)),
    "relpred_transr": (lambda: relpred_transr(120, 8, 6, 3), lambda: relpred_transr(700, 32, 300, 40)),
    "topk_tails": (lambda: topk_tails(3, 2, 16), lambda: topk_tails(150, 40, 48)),
    "link_prediction": (lambda: link_prediction(2), lambda: link_prediction(40)),
    "lazy_adam_transh": (lambda: lazy_adam_transh(30, 16), lambda: lazy_adam_transh(2, 40)),
    "transr_groups": (lambda: transr_groups(30, 16), lambda: transr_groups(3, 48)),
    "transe_counts": (lambda: transe_counts(30, 16), lambda: transe_counts(2, 64)),
    "persistent": (lambda: persistent(4, 2), lambda: persistent(1, 7)),
}


if __name__ == "__main__":
    case, order, path = sys.argv[1:4]
    a, b = CASES[case]
    res = {}
    for i, c in enumerate(order):
        for k, v in (a if c == "A" else b)().items():
            res["%d/%s" % (i, k)] = np.asarray(v)
    np.savez(path, **res)
    print("ok")
