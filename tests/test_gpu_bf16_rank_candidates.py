"""kge_rank_candidates_bf16 (include/kge_mi355.h, "Evaluation on bf16 tables"): the counts of kge_rank_candidates on the widened
tables, from the stored bf16 rows -- every candidate mode, both sides, filtered or not, at the candidate counts around the team
width, whatever the slices, in the fused and in the two-stage form.  One width per rung of csrc/team_shape.hpp; E = 300, R = 4,
n = 37 triples over score_ref.eval_graph's made-up files.  On axis tables the counts are tied to exact integer scores counted in
numpy, without the fp32 kernel."""
import functools

import numpy as np
import pytest

import bf16_eval_rig as rig
import bf16_ref as ref
import score_ref
from bf16_eval_rig import DRAWN, FILTERED, NO_HEAD, TYPED
from gpu_engine import make_engine

pytestmark = pytest.mark.gpu

E, R, N = 300, 4, 37
WIDTHS = rig.MULTIPLE_OF_8_PER_RUNG
SEED = 0x9E3779B97F4A7C15


@functools.lru_cache(maxsize=None)
def graph_and_lists():
    return score_ref.eval_graph(E, R, score_ref.seed_of("bf16-rank-graph")), score_ref.made_up_type_lists(E, R, score_ref.seed_of("bf16-rank-types"))


def import_graph():
    """The filter index and the type lists are the library's, not a table's: import them through a small Config (its own tables
    are not used -- the entry points below take addresses).  Relation 1 has empty type lists."""
    g, lists = graph_and_lists()
    con = make_engine("transe", E, R, 16, 16, score_ref.random_tables("transe", E, R, 16, 16, 1), train=g["train"])
    con.init_evaluation_from_arrays(g["valid"], g["test"], type_lists=lists)
    return con


def queries():
    g, _ = graph_and_lists()
    h, t, r = (x[:N].copy() for x in score_ref.eval_queries(g))
    assert len(h) == N and (r == 1).any()
    return h, t, r


def known_sets():
    g, _ = graph_and_lists()
    tails, heads = {}, {}
    for h, t, r in score_ref.known_triples(g):
        tails.setdefault((h, r), set()).add(t)
        heads.setdefault((t, r), set()).add(h)
    return tails, heads


def per_triple_lists(h, t, r, C, seed):
    """(tail lists, head lists) int64 [N, C]: random ids with, spread over the triples, known tails / heads of the query (the
    filter bites), the target, a repeated id, -1 in the middle and at the end, ids beyond the table; triple 1's lists are all -1."""
    rng = np.random.default_rng(seed)
    known = known_sets()
    out = []
    for side in (0, 1):
        rows = rng.integers(0, E, (N, C))
        for i in range(N):
            fixed, target = (t[i], h[i]) if side else (h[i], t[i])
            row = rows[i]
            for j, v in enumerate(sorted(known[side].get((int(fixed), int(r[i])), ()))[:max(1, C // 4)]):
                row[(3 * j + 1) % C] = v
            if i % 2 == 0:
                row[(i // 2) % C] = target
            if C >= 8:
                row[C // 2] = row[0]
                row[C // 3] = -1
                if i % 4 != 3:
                    row[C - 1] = -1
                row[C // 4] = (E, E + 5, -7)[i % 3]
            if i == 1:
                row[:] = -1
        out.append(rows)
    return out


class Options:
    def __init__(self, **options):
        self.options = options

    def __enter__(self):
        for k, v in self.options.items():
            assert rig.lib().kge_set_option(k.encode(), v) == 0

    def __exit__(self, *exc):
        rig.lib().kge_set_option(b"rankc_fused", 1)
        rig.lib().kge_set_option(b"rankc_slices", 0)


def calls(h, t, r, C, seed):
    """The argument sets of one candidate count: name -> (tail, tail stride, head, head stride, flags) with device lists."""
    tails, heads = per_triple_lists(h, t, r, C, seed)
    shared = np.random.default_rng(seed + 1).integers(0, E, C)
    if C >= 3:
        shared[C // 2], shared[C // 3] = shared[0], -1
    dt, dh, ds = rig.dev(tails, np.int32), rig.dev(heads, np.int32), rig.dev(shared, np.int32)
    out = {"lists": (dt, C, dh, C, 0), "shared list": (ds, 0, ds, 0, 0), "no tail side": (None, 0, dh, C, 0), "no head side": (dt, C, None, 0, 0),
           "drawn": (None, 0, None, 0, DRAWN), "drawn typed": (None, 0, None, 0, DRAWN | TYPED), "drawn tail only": (None, 0, None, 0, DRAWN | NO_HEAD)}
    return out


@functools.lru_cache(maxsize=None)
def random_case(D):
    p = score_ref.random_tables("transe", E, R, D, D, score_ref.seed_of("bf16-rank-tables", D), 3.0)
    return rig.Tables.rounded(p["ent_embeddings"], p["rel_embeddings"])


@pytest.mark.parametrize("D", WIDTHS)
def test_counts_are_the_fp32_kernels_on_the_widened_tables(D):
    con = import_graph()
    tabs = random_case(D)
    L, _ = score_ref.rung_of(D)
    h, t, r = queries()
    dh_, dt_, dr_ = (rig.dev(x, np.int32) for x in (h, t, r))
    bites = counted = 0
    for C in (1, L - 1, L, L + 1, 3 * L + 2):
        for name, (tail, ts, head, hs, flags) in calls(h, t, r, C, 100 + C).items():
            for filt in (FILTERED, 0):
                args = (dh_, dt_, dr_, tail, ts, head, hs, C, flags | filt, SEED)
                rc32, want = rig.rank_candidates(tabs, *args, bf16=False)
                rc, got = rig.rank_candidates(tabs, *args)
                assert rc == 0 and rc32 == 0, (C, name, filt, rc, rc32)
                assert np.array_equal(got, want), (C, name, filt, np.argwhere(got != want)[:5].tolist())
                assert (got >= 0).all()                                 # every element written
                if name == "no tail side" or name == "drawn tail only":
                    assert not got[:, 0 if name == "no tail side" else 1].any()
                if name == "lists":
                    assert not got[1].any()                             # the all -1 lists
                counted += int(got[:, :, 0].sum())
                bites += int(filt and (got[:, :, 1] < got[:, :, 0]).any())
                if not filt:
                    assert np.array_equal(got[:, :, 0], got[:, :, 1])
                if C in (1, L - 1):      # the two-stage form at the short lists too (one slice: nothing to cut)
                    with Options(rankc_fused=0):
                        rc, again = rig.rank_candidates(tabs, *args)
                    assert rc == 0 and np.array_equal(again, want), (C, name, filt, np.argwhere(again != want)[:5].tolist())
                if C != 3 * L + 2:
                    continue
                # the counts depend neither on the slices nor on the form
                for fused in (1, 0):
                    for slices in (1, 3):
                        with Options(rankc_fused=fused, rankc_slices=slices):
                            rc, again = rig.rank_candidates(tabs, *args)
                        assert rc == 0 and np.array_equal(again, want), (name, filt, fused, slices, np.argwhere(again != want)[:5].tolist())
    assert counted > 0 and bites > 0
    del con


def numpy_counts(score, h, t, r, tails, heads):
    """[N, 2, 2] from a score function and the made-up files: strict `<`, the target id and ids outside the table skipped."""
    known = known_sets()
    counts = np.zeros((len(h), 2, 2), np.int64)
    for i in range(len(h)):
        for side, lists in ((0, tails), (1, heads)):
            row = np.asarray(lists if np.ndim(lists) == 1 else lists[i], dtype=np.int64)
            fixed, target = (t[i], h[i]) if side else (h[i], t[i])
            ids = row[(row >= 0) & (row < E)]
            ids = ids[ids != target]
            if len(ids) == 0:
                continue
            fx, rr = np.full(len(ids), fixed), np.full(len(ids), r[i])
            s = score(ids, fx, rr) if side else score(fx, ids, rr)
            s0 = score([h[i]], [t[i]], [r[i]])[0]
            below = s < s0
            kn = np.array([int(c) in known[side].get((int(fixed), int(r[i])), ()) for c in ids], bool)
            counts[i, side] = [below.sum(), (below & ~kn).sum()]
    return counts


@functools.lru_cache(maxsize=None)
def axis_case(D):
    """score_ref.exact_tables' axis tables with two rows rewritten: entity `twin` gets the row of triple 0's tail (its score ties
    with the true triple's: not counted) and entity `zero` an all-zero row.  Swapping one unit vector for another moves the
    integer score by 0 or 2; the zero row takes one unit vector away, so it lands ONE unit beside a target: where that is below,
    it is counted."""
    params = score_ref.exact_tables("transe", E, R, D, D)
    h, t, r = queries()
    twin, zero = [e for e in range(E - 1, 0, -1) if e not in h and e not in t][:2]
    params["ent_embeddings"][twin] = params["ent_embeddings"][t[0]]
    params["ent_embeddings"][zero] = 0.0
    for x in params.values():
        assert np.array_equal(ref.widen(ref.to_bf16(x)).view(np.uint32), x.view(np.uint32))
    return params, rig.Tables(params["ent_embeddings"], params["rel_embeddings"]), twin, zero


@pytest.mark.parametrize("D", WIDTHS)
def test_axis_tables_counts_are_numpy_counts_over_exact_integer_scores(D):
    con = import_graph()
    params, tabs, twin, zero = axis_case(D)
    h, t, r = queries()
    score = lambda a, b, q: score_ref.exact_scores("transe", params, a, b, q, D, D, "own_matrix")
    units = lambda a, b, q: np.rint(score(a, b, q).astype(np.float64) * D).astype(np.int64)       # the integer the score is over D
    everyone = np.arange(E)
    want = numpy_counts(score, h, t, r, everyone, everyone)
    # what the lists hold: a candidate whose row is the target's row (a tie: not counted) and a candidate exactly one unit below
    # its target (counted)
    u0 = units([h[0]], [t[0]], [r[0]])[0]
    assert twin != t[0] and units([h[0]], [twin], [r[0]])[0] == u0
    target_units, zero_units = units(h, t, r), units(h, np.full(N, zero), r)
    one_below = np.nonzero(zero_units == target_units - 1)[0]
    assert len(one_below) and want[:, :, 0].any() and (want[:, :, 1] < want[:, :, 0]).any()
    dh_, dt_, dr_, ev_ = (rig.dev(x, np.int32) for x in (h, t, r, everyone))
    only_zero = rig.dev(np.array([zero]), np.int32)
    rc, got = rig.rank_candidates(tabs, dh_, dt_, dr_, only_zero, 0, None, 0, 1, 0)
    assert rc == 0 and (got[one_below, 0, 0] == 1).all() and np.array_equal(got[:, 0, 0], (zero_units < target_units).astype(np.int64))
    rc, got = rig.rank_candidates(tabs, dh_, dt_, dr_, ev_, 0, ev_, 0, E, FILTERED)
    assert rc == 0 and np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    # the tie alone: a list of the twin only counts nothing on the tail side of triple 0; without the tie rule it would not be 0
    one = rig.dev(np.array([twin]), np.int32)
    rc, got = rig.rank_candidates(tabs, dh_, dt_, dr_, one, 0, None, 0, 1, 0)
    assert rc == 0 and got[0, 0, 0] == 0 and np.array_equal(got, numpy_counts(score, h, t, r, np.array([twin]), np.zeros(0, np.int64)))
    tails, heads = per_triple_lists(h, t, r, 37, 5)
    rc, got = rig.rank_candidates(tabs, dh_, dt_, dr_, rig.dev(tails, np.int32), 37, rig.dev(heads, np.int32), 37, 37, FILTERED)
    assert rc == 0 and np.array_equal(got, numpy_counts(score, h, t, r, tails, heads))
    del con


def test_edges_and_refusals():
    import torch
    con = import_graph()
    D, C = 24, 17
    tabs = random_case(D)
    h, t, r = queries()
    tails, heads = per_triple_lists(h, t, r, C, 1)
    d = lambda a: rig.dev(a, np.int32)
    dh_, dt_, dr_, tl, hl = d(h), d(t), d(r), d(tails), d(heads)
    rc, base = rig.rank_candidates(tabs, dh_, dt_, dr_, tl, C, hl, C, C, FILTERED)
    assert rc == 0 and base[:, :, 0].any()
    counts = torch.full((N, 2, 2), rig.FILL, dtype=torch.int64, device="cuda")
    untouched = lambda: bool((counts == rig.FILL).all().item())
    call = lambda *a, **kw: rig.rank_candidates(tabs, *a, counts=counts, **kw)
    # n == 0: nothing written; n_cand == 0: zeros, with lists and drawn
    assert call(dh_, dt_, dr_, tl, C, hl, C, C, FILTERED, n=0)[0] == 0 and untouched()
    assert call(dh_, dt_, dr_, tl, 0, hl, 0, 0, FILTERED)[0] == 0 and not counts.any().item()
    counts.fill_(rig.FILL)
    assert call(dh_, dt_, dr_, None, 0, None, 0, 0, FILTERED | DRAWN)[0] == 0 and not counts.any().item()
    # disabled triples: zeros, the others as before, KGE_OK -- in both forms, drawn lists included
    bh, bt, br = h.copy(), t.copy(), r.copy()
    bh[3], bt[4], br[5], bh[6] = -1, E, R, 2 ** 31 - 1
    keep = np.ones(N, bool); keep[3:7] = False
    counts.fill_(rig.FILL)
    rc, got = call(d(bh), d(bt), d(br), tl, C, hl, C, C, FILTERED)
    assert rc == 0 and not got[3:7].any() and np.array_equal(got[keep], base[keep]) and base[3:7].any()
    _, drawn = rig.rank_candidates(tabs, dh_, dt_, dr_, None, 0, None, 0, C, FILTERED | DRAWN, 7)
    for fused in (0, 1):
        with Options(rankc_fused=fused):
            counts.fill_(rig.FILL)
            rc, got = call(d(bh), d(bt), d(br), None, 0, None, 0, C, FILTERED | DRAWN, 7)
        assert rc == 0 and not got[3:7].any() and np.array_equal(got[keep], drawn[keep])
    # refusals: the limits of kge_bf16_eval_supported, then null and inconsistent arguments; the output stays as it was
    counts.fill_(rig.FILL)
    for desc in (rig.desc(E, R, 12), rig.desc(E, R, 1032), rig.desc(E, R, D, model=1), rig.desc(E, R, D, 8)):
        assert call(dh_, dt_, dr_, tl, C, hl, C, C, FILTERED, d=desc)[0] == rig.KGE_ERR_UNSUPPORTED and untouched(), (desc.model, desc.ent_dim)
    for kw in (dict(ent=None), dict(rel=None)):
        assert call(dh_, dt_, dr_, tl, C, hl, C, C, FILTERED, **kw)[0] == rig.KGE_ERR_BAD_ARG and untouched(), kw
    bad = [(None, dt_, dr_, tl, C, hl, C, C, FILTERED), (dh_, None, dr_, tl, C, hl, C, C, FILTERED), (dh_, dt_, None, tl, C, hl, C, C, FILTERED),
           (dh_, dt_, dr_, tl, C, hl, C, -1, FILTERED), (dh_, dt_, dr_, None, 0, None, 0, C, FILTERED), (dh_, dt_, dr_, tl, C, None, 0, C, FILTERED | DRAWN),
           (dh_, dt_, dr_, tl, C, hl, C, C, FILTERED | TYPED), (dh_, dt_, dr_, tl, C, hl, C, C, NO_HEAD), (dh_, dt_, dr_, tl, C - 1, hl, C, C, FILTERED),
           (dh_, dt_, dr_, tl, C, hl, C, C, 16)]
    for args in bad:
        assert call(*args, n=N)[0] == rig.KGE_ERR_BAD_ARG and untouched(), args[3:]
    assert call(dh_, dt_, dr_, tl, C, hl, C, C, FILTERED, n=-1)[0] == rig.KGE_ERR_BAD_ARG and untouched()
    del con
