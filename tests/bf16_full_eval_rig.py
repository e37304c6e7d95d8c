"""Shared by the GPU tests of the full-entity evaluators on stored bf16 tables (include/kge_mi355.h, "Evaluation on bf16 tables":
kge_rank_triples_bf16, kge_topk_entities_bf16): the made-up evaluation files, the two table families, and the two pairs of entry
points called through the C ABI into pre-filled buffers.  bf16_eval_rig supplies the tables' two forms on the device."""
import ctypes
import functools

import numpy as np

import bf16_eval_rig as rig
import score_ref
from gpu_engine import make_engine

R = 5
FILL = rig.FILL
TOPK_TABLE_DEFAULT = 1 << 30          # csrc/engine.hpp


@functools.lru_cache(maxsize=None)
def graph_and_lists(E):
    return (score_ref.eval_graph(E, R, score_ref.seed_of("bf16-full-graph", E)),
            score_ref.made_up_type_lists(E, R, score_ref.seed_of("bf16-full-types", E)))


def import_graph(E):
    """The filter index and the type lists are the library's, not a table's: import them through a small Config whose own tables
    are not used.  Relation 1 has empty type lists."""
    g, lists = graph_and_lists(E)
    con = make_engine("transe", E, R, 16, 16, score_ref.random_tables("transe", E, R, 16, 16, 1), train=g["train"])
    con.init_evaluation_from_arrays(g["valid"], g["test"], type_lists=lists)
    return con


@functools.lru_cache(maxsize=None)
def triples(E, n):
    """n evaluation triples of mixed relations, two of them repeated."""
    h, t, r = (x[:n].copy() for x in score_ref.eval_queries(graph_and_lists(E)[0]))
    for x in (h, t, r):
        x[n - 1], x[n // 2] = x[0], x[5]
    assert len(h) == n and len(set(r.tolist())) == R
    return h, t, r


def special_rows(E, h, t):
    """Ids for family (a)'s rows: zero and tiny are a queried tail and head (their clipped norms reach the request vectors too),
    inf, nan and twin are candidates only; twin gets the row of triple 0's tail, a target."""
    used = set(h.tolist()) | set(t.tolist())
    free = [e for e in range(E - 1, 0, -1) if e not in used]
    zero, tiny = int(t[2]), int(h[3])
    assert zero != tiny and zero != int(t[0]) and tiny != int(t[0])
    return dict(zero=zero, tiny=tiny, inf=free[0], nan=free[1], twin=free[2])


@functools.lru_cache(maxsize=None)
def special_tables(E, D, n):
    """Family (a): normal draws rounded to bf16, with an all-zero row (clipped norm), a row of 2^-70 (its squares underflow: clipped
    too), a row with an inf, a row with a NaN, and two identical rows, one of them a target."""
    p = score_ref.random_tables("transe", E, R, D, D, score_ref.seed_of("bf16-full-tables", E, D), 3.0)
    ent, rel = p["ent_embeddings"].copy(), p["rel_embeddings"]
    h, t, _ = triples(E, n)
    rows = special_rows(E, h, t)
    ent[rows["zero"]] = 0.0
    ent[rows["tiny"]] = np.float32(2.0 ** -70)
    ent[rows["inf"], D // 2] = np.inf
    ent[rows["nan"], D - 1] = np.nan
    ent[rows["twin"]] = ent[t[0]]
    return rig.Tables.rounded(ent, rel), rows


@functools.lru_cache(maxsize=None)
def tie_tables(E, D):
    """Family (b): every element of both tables is +1 or -1 (bf16 values).  All norms are equal and a score is a multiple of
    1 / (D sqrt D) before rounding: a candidate's score differs from a target's by rounding order only, or by a whole step."""
    rng = np.random.default_rng(score_ref.seed_of("bf16-full-ties", E, D))
    sign = lambda shape: (rng.integers(0, 2, shape) * 2 - 1).astype(np.float32)
    return rig.Tables(sign((E, D)), sign((R, D)))


def near_ties(tabs, h, t, r, ulps=4):
    """How many (triple, side, candidate) have a row unlike the target's and an fp64 score within `ulps` float32 ulps of the true
    triple's fp64 score."""
    ent, rel = score_ref.l2n(tabs.ent32.astype(np.float64)), score_ref.l2n(tabs.rel32.astype(np.float64))
    count = 0
    for i in range(len(h)):
        true = np.abs(ent[h[i]] + rel[r[i]] - ent[t[i]]).mean()
        tol = ulps * float(np.spacing(np.float32(true)))
        for fixed, target, sign in ((ent[h[i]] + rel[r[i]], t[i], -1.0), (rel[r[i]] - ent[t[i]], h[i], 1.0)):
            s = np.abs(fixed[None, :] + sign * ent).mean(1)
            unlike = (tabs.ent32 != tabs.ent32[target][None, :]).any(1)
            count += int((unlike & (np.abs(s - true) <= tol)).sum())
    return count


class Options:
    """Engine options for the length of a `with` block, then back to their defaults."""
    DEFAULTS = {"rank_slices": 0, "topk_table_max_bytes": TOPK_TABLE_DEFAULT}

    def __init__(self, **options):
        self.options = options

    def __enter__(self):
        for k, v in self.options.items():
            assert rig.lib().kge_set_option(k.encode(), v) == 0

    def __exit__(self, *exc):
        for k in self.options:
            rig.lib().kge_set_option(k.encode(), self.DEFAULTS[k])


def rank_triples(tabs, h, t, r, test_head, bf16=True, n=None, counts=None, d=None, ent=Ellipsis, rel=Ellipsis):
    """kge_rank_triples_bf16 on the stored tables or kge_rank_triples on the widened ones; h, t, r device tensors or None ->
    (return code, counts int64 numpy [n, 2, 4] from a buffer pre-filled with FILL)."""
    import torch
    L = rig.lib()
    n = max(len(x) for x in (h, t, r) if x is not None) if n is None else n
    if counts is None:
        counts = torch.full((max(n, 1), 2, 4), FILL, dtype=torch.int64, device="cuda")
    d = tabs.desc if d is None else d
    tail = (rig.ptr(h), rig.ptr(t), rig.ptr(r), n, test_head, rig.ptr(counts), None)
    if bf16:
        rc = L.kge_rank_triples_bf16(ctypes.byref(d), rig.ptr(tabs.ent_b if ent is Ellipsis else ent), rig.ptr(tabs.rel_b if rel is Ellipsis else rel), *tail)
    else:
        rc = L.kge_rank_triples(ctypes.byref(d), tabs.fp32_ptrs(), *tail)
    torch.cuda.synchronize()
    L.kge_clear_error()
    return rc, counts.cpu().numpy()


def topk(tabs, fixed, rel_ids, head, k, flags, bf16=True, n=None, d=None, ent=Ellipsis, rel=Ellipsis, out=None):
    """kge_topk_entities_bf16 / kge_topk_entities; fixed, rel_ids, head device tensors -> (return code, ids int32 numpy [n, k],
    scores as uint32 bits [n, k]) from buffers pre-filled with FILL."""
    import torch
    L = rig.lib()
    n = max(len(x) for x in (fixed, rel_ids, head) if x is not None) if n is None else n
    ids, scores = out if out is not None else (torch.full((max(n, 1), k), FILL, dtype=torch.int32, device="cuda"),
                                               torch.full((max(n, 1), k), float(FILL), dtype=torch.float32, device="cuda"))
    d = tabs.desc if d is None else d
    tail = (rig.ptr(fixed), rig.ptr(rel_ids), rig.ptr(head), n, k, flags, rig.ptr(ids), rig.ptr(scores), None)
    if bf16:
        rc = L.kge_topk_entities_bf16(ctypes.byref(d), rig.ptr(tabs.ent_b if ent is Ellipsis else ent), rig.ptr(tabs.rel_b if rel is Ellipsis else rel), *tail)
    else:
        rc = L.kge_topk_entities(ctypes.byref(d), tabs.fp32_ptrs(), *tail)
    torch.cuda.synchronize()
    L.kge_clear_error()
    return rc, ids.cpu().numpy(), scores.cpu().numpy().view(np.uint32)


def first_diff(a, b):
    return np.argwhere(np.asarray(a) != np.asarray(b))[:5].tolist()
