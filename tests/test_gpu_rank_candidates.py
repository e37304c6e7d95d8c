"""kge_rank_candidates / Config.rank_candidates / rank_triples_sampled: ranks against candidate lists (csrc/rank_cand.hip), on
tests/score_ref.py's rig.  Axis tables: every count is an exact integer from exact_scores.  Random tables: the fp64 definition
wherever fp64 can tell (a query is set aside only when a LISTED candidate lies within BAND of the target), and exactly the
counts computed in numpy from test_step's scores over the spelled-out (triple, candidate) pairs -- kge_predict's bits -- for the
fused kernel and the two-stage form alike, whatever the slices.  Drawn lists against an independent restatement of the hash."""
import ctypes
import functools
import os

import numpy as np
import pytest

import score_ref
from conftest import parity_report
from gpu_engine import make_engine
from openkeonspark_amd import rank_eval
from score_ref import BAND, EVAL_CASES, MAX_ASIDE

pytestmark = pytest.mark.gpu

KGE_ERR_NO_DATASET, KGE_ERR_BAD_ARG, KGE_ERR_UNSUPPORTED = -2, -3, -4
FILTERED, DRAWN, TYPED, NO_HEAD = 1, 2, 4, 8
LIST_LENGTHS = (1, 17, 37, 65, 300)          # 300 = every entity of the axis tables once
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def case_of(model, De, Dr, kind):
    """One reference per case, shared by the tests and left unchanged (Evaluators caches the candidate scores per query)."""
    return score_ref.eval_case(model, De, Dr, kind)


def engine_for(case, model, De, Dr):
    g = case["graph"]
    con = make_engine(model, g["E"], g["R"], De, Dr, case["params"], train=g["train"])
    con.init_evaluation_from_arrays(g["valid"], g["test"], type_lists=case["lists"])
    return con


def per_triple_lists(ev, h, t, r, C, seed):
    """(tail lists, head lists) int64 [n, C].  C == E: every entity once, in a different order per triple.  Otherwise random ids
    with, spread over the triples: the target, known tails / heads of the query, a repeated id, -1 in the middle and at the
    end, ids beyond the table (skipped like -1); triple 1's lists are all -1.  C == 1 cycles target / known / random / -1."""
    rng = np.random.default_rng(seed)
    E, n = ev.E, len(h)
    out = []
    for side in (0, 1):
        rows = np.empty((n, C), np.int64)
        for i in range(n):
            fixed, target = (t[i], h[i]) if side else (h[i], t[i])
            known = sorted((ev.known_heads if side else ev.known_tails).get((int(fixed), int(r[i])), ()))
            if C == E:
                rows[i] = rng.permutation(E)
                continue
            row = rng.integers(0, E, C)
            if C == 1:
                row[0] = (target, known[0] if known else 0, row[0], -1)[i % 4]
            else:
                for j, v in enumerate(known[:max(1, C // 4)]):
                    row[(3 * j + 1) % C] = v
                if i % 2 == 0:
                    row[(i // 2) % C] = target
                if C >= 8:
                    row[C // 2] = row[0]                        # a repeated id: counted twice
                    row[C // 3] = -1                            # padding in the middle ...
                    if i % 4 != 3:
                        row[C - 1] = -1                         # ... and at the end
                    row[C // 4] = (E, E + 5, -7)[i % 3]         # outside the table
            if i == 1:
                row[:] = -1
            rows[i] = row
        out.append(rows)
    return out


def shared_list(E, C, seed):
    row = np.random.default_rng(seed).integers(0, E, C)
    row[C // 2], row[C // 3], row[C - 1] = row[0], -1, -1
    return row


def list_counts(ev, h, t, r, tail_lists, head_lists, band=0.0):
    """The two counts from Evaluators.entity_scores for arbitrary lists ([n, C], a shared [C], or None): -> (int64 [n, 2, 2],
    aside bool [n, 2]: a listed candidate other than the target lies within `band`, relative, of the target's score)."""
    n = len(h)
    counts, aside = np.zeros((n, 2, 2), np.int64), np.zeros((n, 2), bool)
    for i in range(n):
        for side, lists in ((0, tail_lists), (1, head_lists)):
            if lists is None:
                continue
            row = np.asarray(lists if np.ndim(lists) == 1 else lists[i], dtype=np.int64)
            fixed, target = (t[i], h[i]) if side else (h[i], t[i])
            s, known, _ = ev.entity_scores(fixed, r[i], side == 1)
            ids = row[(row >= 0) & (row < ev.E)]
            ids = ids[ids != target]
            below = s[ids] < s[target]
            counts[i, side] = [below.sum(), (below & ~known[ids]).sum()]
            if band:
                aside[i, side] = bool((np.abs(s[ids] - s[target]) <= band * abs(s[target])).any())
    return counts, aside


def predict_counts(con, graph, h, t, r, tail_lists, head_lists):
    """The same two counts in numpy from con.test_step over the spelled-out (triple, candidate) pairs and the true triples, the
    filter from a Python set.  One test_step call per relation: kge_predict projects a TransR call by its first triple's matrix."""
    known, E, n = score_ref.known_triples(graph), graph["E"], len(h)
    rows = []                                            # (triple, side, candidate or -1 for the true triple, h, t, r)
    for i in range(n):
        for side, lists in ((0, tail_lists), (1, head_lists)):
            if lists is None:
                continue
            row = np.asarray(lists if np.ndim(lists) == 1 else lists[i], dtype=np.int64)
            rows.append((i, side, -1, h[i], t[i], r[i]))
            for c in row[(row >= 0) & (row < E)].tolist():
                rows.append((i, side, c, c if side else h[i], t[i] if side else c, r[i]))
    rows = np.asarray(rows, dtype=np.int64)
    sc = np.empty(len(rows), np.float32)
    for q in np.unique(rows[:, 5]).tolist():
        m = rows[:, 5] == q
        sc[m] = np.asarray(con.test_step(rows[m, 3], rows[m, 4], rows[m, 5])).reshape(-1)
    counts = np.zeros((n, 2, 2), np.int64)
    target_score = {(i, side): s for (i, side, c, *_), s in zip(rows.tolist(), sc) if c < 0}
    for (i, side, c, hh, tt, rr), s in zip(rows.tolist(), sc):
        if c < 0 or c == (h[i] if side else t[i]) or not (s < target_score[i, side]):
            continue
        counts[i, side, 0] += 1
        counts[i, side, 1] += (hh, tt, rr) not in known
    return counts


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,De,Dr", EVAL_CASES)
def test_axis_tables_exact_integers(model, De, Dr):
    case = case_of(model, De, Dr, "exact")
    g, ev = case["graph"], case["ev"]
    con = engine_for(case, model, De, Dr)
    h, t, r = score_ref.eval_queries(g)
    E, n = g["E"], len(h)
    assert E == 300
    bites = False
    for C in LIST_LENGTHS:
        tails, heads = per_triple_lists(ev, h, t, r, C, score_ref.seed_of("lists", C))
        want, _ = list_counts(ev, h, t, r, tails, heads)
        got, metrics = con.rank_candidates(h, t, r, tails, heads)
        assert got.dtype == np.int64 and got.shape == (n, 2, 2)
        assert np.array_equal(got, want), (C, np.argwhere(got != want)[:5].tolist())
        assert not got[1].any() or C == E                     # the all -1 lists
        assert metrics == rank_eval.normalise(rank_eval.cand_sums(want), n)
        bites |= bool((want[:, :, 1] < want[:, :, 0]).any())
        if C == 37:
            assert want[:, :, 0].any()
            raw, _ = con.rank_candidates(h, t, r, tails, heads, filtered=False)
            assert np.array_equal(raw[:, :, 0], want[:, :, 0]) and np.array_equal(raw[:, :, 1], want[:, :, 0])
            one, m1 = con.rank_candidates(h, t, r, head_candidates=heads)              # one side: the other stays zero
            assert np.array_equal(one[:, 1], want[:, 1]) and not one[:, 0].any() and not any(k.startswith("r") for k in m1)
    assert bites                                              # the filter bites: column 1 < column 0 for some row
    # one list shared by all triples (stride 0)
    row = shared_list(E, 37, 5)
    want, _ = list_counts(ev, h, t, r, row, row)
    got, _ = con.rank_candidates(h, t, r, row, row)
    assert np.array_equal(got, want) and want[:, :, 0].any()
    # every entity, as a shared list and as per-triple permutations: rank_triples's raw and filtered columns
    full, _ = con.rank_triples(h, t, r)
    got, _ = con.rank_candidates(h, t, r, np.arange(E), np.arange(E))
    assert np.array_equal(got, full[:, :, :2])
    tails, heads = per_triple_lists(ev, h, t, r, E, 9)
    assert np.array_equal(con.rank_candidates(h, t, r, tails, heads)[0], full[:, :, :2])
    assert np.array_equal(full[:, :, :2], ev.rank_counts(h, t, r)[0][:, :, :2])


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,De,Dr", EVAL_CASES)
def test_random_tables_agree_with_fp64_wherever_fp64_can_tell(model, De, Dr):
    case = case_of(model, De, Dr, "random")
    g, ev = case["graph"], case["ev"]
    con = engine_for(case, model, De, Dr)
    h, t, r = score_ref.eval_queries(g)
    shares = {}
    for C in LIST_LENGTHS:
        tails, heads = per_triple_lists(ev, h, t, r, C, score_ref.seed_of("lists", C))
        want, aside = list_counts(ev, h, t, r, tails, heads, BAND)
        got, _ = con.rank_candidates(h, t, r, tails, heads)
        shares[C] = float(aside.mean())
        assert aside.mean() <= MAX_ASIDE, (C, aside.mean())
        assert np.array_equal(got[~aside], want[~aside]), (C, np.argwhere((got != want).any(-1) & ~aside)[:5].tolist())
        if C == 65:
            assert (want[:, :, 1] < want[:, :, 0]).any() and want[:, :, 1].any()
    parity_report("rank_candidates[%s De=%d Dr=%d]" % (model, De, Dr), set_aside_share=shares, cap=MAX_ASIDE)


# 3 ------------------------------------------------------------------------------------------------------------------------
def with_options(con, **options):
    class Ctx:
        def __enter__(self):
            for k, v in options.items():
                assert con.lib.kge_set_option(k.encode(), v) == 0

        def __exit__(self, *exc):
            con.lib.kge_set_option(b"rankc_fused", 1)
            con.lib.kge_set_option(b"rankc_slices", 0)
    return Ctx()


@pytest.mark.parametrize("model,De,Dr", EVAL_CASES)
def test_counts_are_those_of_kge_predicts_scores(model, De, Dr):
    case = case_of(model, De, Dr, "random")
    g, ev = case["graph"], case["ev"]
    con = engine_for(case, model, De, Dr)
    h, t, r = score_ref.eval_queries(g)
    tails, heads = per_triple_lists(ev, h, t, r, 37, 3)
    want = predict_counts(con, g, h, t, r, tails, heads)
    assert want[:, :, 0].any() and (want[:, :, 1] < want[:, :, 0]).any()
    got, _ = con.rank_candidates(h, t, r, tails, heads)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    for fused in (1, 0):
        for slices in (1, 3, 7):
            with with_options(con, rankc_fused=fused, rankc_slices=slices):
                again, _ = con.rank_candidates(h, t, r, tails, heads)
            assert np.array_equal(again, want), (fused, slices, np.argwhere(again != want)[:5].tolist())
    with with_options(con, rankc_fused=0):
        drawn2, _ = con.rank_triples_sampled(h, t, r, 23, seed=4)
    assert np.array_equal(con.rank_triples_sampled(h, t, r, 23, seed=4)[0], drawn2)


@pytest.mark.parametrize("model,De,Dr", [c for c in EVAL_CASES if c[0] != "transr"])
def test_candidates_within_an_ulp_of_the_true_triple(model, De, Dr):
    """The upper half of the entity rows become copies of the queries' tail and head rows with up to three elements moved by one
    ulp, so their scores lie within a few ulps of a true triple's, on either side or tied: a count then hangs on the last bit
    of every score, and the fused kernel (its products written out as kge_predict's compiled form contracts them) must still give
    the two-stage form's counts, which are kge_predict's own kernel's."""
    case = case_of(model, De, Dr, "random")
    g = case["graph"]
    con = engine_for(case, model, De, Dr)
    h, t, r = score_ref.eval_queries(g)
    E = g["E"]
    rng = np.random.default_rng(17)
    ent = np.array(case["params"]["ent_embeddings"], dtype=np.float32)
    aux = np.array(case["params"]["ent_transfer"], dtype=np.float32) if model == "transd" else None
    src = np.concatenate([t, h])
    for j in range(E // 2, E):
        e = src[(j - E // 2) % len(src)]
        row = ent[e].copy()
        cols = rng.choice(De, int(rng.integers(0, min(4, De + 1))), replace=False)
        row[cols] = np.nextafter(row[cols], np.where(rng.random(len(cols)) < 0.5, -np.inf, np.inf).astype(np.float32))
        ent[j] = row
        if aux is not None:
            aux[j] = aux[e]
    con.set_parameters_by_name("ent_embeddings", ent)
    if aux is not None:
        con.set_parameters_by_name("ent_transfer", aux)
    everyone = np.arange(E)
    got, _ = con.rank_candidates(h, t, r, everyone, everyone)
    with with_options(con, rankc_fused=0):
        want, _ = con.rank_candidates(h, t, r, everyone, everyone)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert np.array_equal(got[:12], predict_counts(con, g, h[:12], t[:12], r[:12], everyone, everyone))


# 4 ------------------------------------------------------------------------------------------------------------------------
def restated_draw(seed, i, s, k, length):
    """The hash of include/kge_mi355.h (KGE_RANKC_DRAWN) in unbounded Python integers reduced mod 2^64."""
    c = ((2 * i + s) << 32) | k
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * length) >> 32


def restated_lists(seed, r, C, E, type_lists=None):
    """(tail lists, head lists) int64 [n, C]; with type_lists = (head_off, head_ids, tail_off, tail_ids) the typed draw."""
    out = []
    for side in (0, 1):
        rows = np.empty((len(r), C), np.int64)
        for i, q in enumerate(np.asarray(r).tolist()):
            ids = None
            if type_lists is not None:
                off, lst = (type_lists[0], type_lists[1]) if side else (type_lists[2], type_lists[3])
                ids = lst[off[q]:off[q + 1]]
            for k in range(C):
                rows[i, k] = restated_draw(seed, i, side, k, E) if ids is None or len(ids) == 0 else ids[restated_draw(seed, i, side, k, len(ids))]
        out.append(rows)
    return out


@pytest.mark.parametrize("model,De,Dr", [("transe", 24, 24), ("transd", 200, 200), ("transr", 33, 50)])
def test_drawn_lists(model, De, Dr):
    case = case_of(model, De, Dr, "random")
    g = case["graph"]
    con = engine_for(case, model, De, Dr)
    h, t, r = score_ref.eval_queries(g)
    E, n, C, seed = g["E"], len(h), 19, 0x9E3779B97F4A7C15
    tails, heads = restated_lists(seed, r, C, E)
    assert np.array_equal(con.sampled_candidates(n, C, seed, 0), tails) and np.array_equal(con.sampled_candidates(n, C, seed, 1), heads)
    assert tails.min() >= 0 and heads.max() < E
    want, want_metrics = con.rank_candidates(h, t, r, tails, heads)
    got, metrics = con.rank_triples_sampled(h, t, r, C, seed=seed)
    assert np.array_equal(got, want) and metrics == want_metrics and got[:, :, 0].any() and got[:, 1].any()
    again, _ = con.rank_triples_sampled(h, t, r, C, seed=seed)
    assert np.array_equal(again, got)                                            # the same seed: the same lists, the same counts
    other = restated_lists(seed + 1, r, C, E)
    assert not np.array_equal(other[0], tails) and not np.array_equal(other[1], heads)
    assert np.array_equal(con.rank_triples_sampled(h, t, r, C, seed=seed + 1)[0], con.rank_candidates(h, t, r, *other)[0])
    tail_only, m_tail = con.rank_triples_sampled(h, t, r, C, seed=seed, test_head=False)
    assert np.array_equal(tail_only[:, 0], want[:, 0]) and not tail_only[:, 1].any() and "l_filter_tot" not in m_tail
    raw, _ = con.rank_triples_sampled(h, t, r, C, seed=seed, filtered=False)
    assert np.array_equal(raw[:, :, 0], want[:, :, 0]) and np.array_equal(raw[:, :, 1], want[:, :, 0])
    # typed draws: from the relation's tail / head type list; relation 1 has none and takes the untyped draw
    lists = case["lists"]
    for got_l, want_l in zip(con.type_constraints(), lists):
        assert np.array_equal(got_l, want_l)
    ty_tails, ty_heads = restated_lists(seed, r, C, E, lists)
    assert (np.asarray(r) == 1).any() and np.array_equal(ty_tails[np.asarray(r) == 1], tails[np.asarray(r) == 1])
    head_mask, tail_mask = score_ref.type_masks(lists, E, g["R"])
    for i, q in enumerate(np.asarray(r).tolist()):
        if q != 1:
            assert tail_mask[q, ty_tails[i]].all() and head_mask[q, ty_heads[i]].all()
    assert np.array_equal(con.sampled_candidates(n, C, seed, 0, r=r, type_constrained=True), ty_tails)
    assert np.array_equal(con.sampled_candidates(n, C, seed, 1, r=r, type_constrained=True), ty_heads)
    assert not np.array_equal(ty_tails, tails)
    got, _ = con.rank_triples_sampled(h, t, r, C, seed=seed, type_constrained=True)
    assert np.array_equal(got, con.rank_candidates(h, t, r, ty_tails, ty_heads)[0])
    # the validation check: rank_triples_sampled on the validation triples
    vh, vt, vr = g["valid"]
    want, want_metrics = con.rank_triples_sampled(vh, vt, vr, C, seed=3)
    got, metrics = con.validation_link_prediction(candidates=C, seed=3)
    assert np.array_equal(got, want) and metrics == want_metrics and got.shape == (len(vh), 2, 2)
    idx = (np.arange(7) * len(vh)) // 7
    s7, _ = con.validation_link_prediction(sample=7, candidates=C, seed=3, test_head=False)
    assert np.array_equal(s7, con.rank_triples_sampled(vh[idx], vt[idx], vr[idx], C, seed=3, test_head=False)[0])
    assert con.validation_link_prediction()[0].shape == (len(vh), 2, 4)          # candidates = 0: every entity, as before
    # one process, no process group: the collective form is the plain one
    assert np.array_equal(con.rank_triples_sampled_distributed(h, t, r, C, seed=seed)[0], con.rank_triples_sampled(h, t, r, C, seed=seed)[0])
    # a slice of the triples ranked with its global offset gives the slice of the whole call's counts
    import torch
    dev = torch.from_numpy(np.stack([h, t, r]).astype(np.int32)).to(con.device)
    part = rank_eval.rank_candidates_device(con, dev[:, 11:40].contiguous(), None, None, C, FILTERED | DRAWN, seed, first=11)
    assert np.array_equal(part, con.rank_triples_sampled(h, t, r, C, seed=seed)[0][11:40])


# 5 ------------------------------------------------------------------------------------------------------------------------
def raw_call(con, h, t, r, n, tail, tail_stride, head, head_stride, C, flags, seed, counts, desc=None):
    import torch
    ptr = lambda x: None if x is None else x.data_ptr()
    rc = con.lib.kge_rank_candidates(ctypes.byref(desc if desc is not None else con._desc), con._tab_ptrs, ptr(h), ptr(t), ptr(r), n,
                                     ptr(tail), tail_stride, ptr(head), head_stride, C, flags, seed, ptr(counts), con._stream())
    torch.cuda.synchronize()
    return rc


def test_edges_through_the_c_interface(tmp_path):
    import torch
    import openkeonspark_amd as pkg
    model, De, Dr = "transh", 24, 24
    case = case_of(model, De, Dr, "random")
    g, ev = case["graph"], case["ev"]
    con = engine_for(case, model, De, Dr)
    L = con.lib
    hh, tt, rr = score_ref.eval_queries(g)
    n, C, E = len(hh), 17, g["E"]
    tails, heads = per_triple_lists(ev, hh, tt, rr, C, 1)
    base, _ = con.rank_candidates(hh, tt, rr, tails, heads)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(con.device)
    h, t, r, dt_, dh_ = dev(hh), dev(tt), dev(rr), dev(tails), dev(heads)
    counts = torch.full((n, 2, 2), -9, dtype=torch.int64, device=con.device)
    untouched = lambda: bool((counts == -9).all().item())
    fresh = lambda: counts.fill_(-9)
    # the plain call, and a list as a device tensor through Config (int32 and int64)
    assert raw_call(con, h, t, r, n, dt_, C, dh_, C, C, FILTERED, 0, counts) == 0
    assert np.array_equal(counts.cpu().numpy(), base)
    assert np.array_equal(con.rank_candidates(hh, tt, rr, dt_, dh_.long())[0], base)
    assert np.array_equal(con.rank_candidates(hh, tt, rr, dt_[0], None)[0], con.rank_candidates(hh, tt, rr, tails[0], None)[0])
    # n == 0 and n_cand == 0
    fresh()
    assert raw_call(con, h, t, r, 0, dt_, C, dh_, C, C, FILTERED, 0, counts) == 0 and untouched()
    assert raw_call(con, h, t, r, n, dt_, 0, dh_, 0, 0, FILTERED, 0, counts) == 0 and not counts.any().item()
    fresh()
    assert raw_call(con, h, t, r, n, None, 0, None, 0, 0, FILTERED | DRAWN, 0, counts) == 0 and not counts.any().item()
    empty, met = con.rank_candidates([], [], [], np.zeros((0, 5), np.int64), None)
    assert empty.shape == (0, 2, 2) and empty.dtype == np.int64 and "r_filter_tot" in met
    assert not con.rank_triples_sampled(hh, tt, rr, 0)[0].any()
    # a disabled triple: its counts stay zero, the others are ranked, KGE_OK
    bad_h, bad_t, bad_r = hh.copy(), tt.copy(), rr.copy()
    bad_h[3], bad_t[4], bad_r[5], bad_h[6] = E, -1, g["R"], 2 ** 31 - 1
    fresh()
    assert raw_call(con, dev(bad_h), dev(bad_t), dev(bad_r), n, dt_, C, dh_, C, C, FILTERED, 0, counts) == 0
    got = counts.cpu().numpy()
    keep = np.ones(n, bool); keep[3:7] = False
    assert not got[3:7].any() and np.array_equal(got[keep], base[keep]) and base[3:7].any()
    for fused in (0, 1):                                  # the same in both forms, drawn lists included
        with with_options(con, rankc_fused=fused):
            fresh()
            assert raw_call(con, dev(bad_h), dev(bad_t), dev(bad_r), n, None, 0, None, 0, C, FILTERED | DRAWN, 7, counts) == 0
            got = counts.cpu().numpy()
            assert not got[3:7].any() and np.array_equal(got[keep], con.rank_triples_sampled(hh, tt, rr, C, seed=7)[0][keep])
    # null and inconsistent arguments: KGE_ERR_BAD_ARG, the output untouched
    fresh()
    bad = [(None, t, r, n, dt_, C, dh_, C, C, FILTERED), (h, None, r, n, dt_, C, dh_, C, C, FILTERED), (h, t, None, n, dt_, C, dh_, C, C, FILTERED),
           (h, t, r, -1, dt_, C, dh_, C, C, FILTERED), (h, t, r, n, dt_, C, dh_, C, -1, FILTERED),
           (h, t, r, n, None, 0, None, 0, C, FILTERED),                      # no list and no DRAWN
           (h, t, r, n, dt_, C, None, 0, C, FILTERED | DRAWN),               # a list with DRAWN
           (h, t, r, n, dt_, C, dh_, C, C, FILTERED | TYPED),                # TYPED / NO_HEAD without DRAWN
           (h, t, r, n, dt_, C, dh_, C, C, NO_HEAD),
           (h, t, r, n, dt_, C - 1, dh_, C, C, FILTERED),                    # a stride shorter than the list
           (h, t, r, n, dt_, C, dh_, C, C, 16),                              # an unknown flag
           (None, t, r, 0, dt_, C, dh_, C, C, FILTERED)]                     # null pointers are refused with n == 0 too
    for args in bad:
        assert raw_call(con, *args, 0, counts) == KGE_ERR_BAD_ARG and untouched(), args[3:]
    assert raw_call(con, h, t, r, n, dt_, C, dh_, C, C, FILTERED, 0, None) == KGE_ERR_BAD_ARG
    assert raw_call(con, h, t, r, n, dt_, C, dh_, C, C, FILTERED, 0, counts, desc=con._desc_with(ent_dim=1025)) == KGE_ERR_UNSUPPORTED and untouched()
    L.kge_clear_error()
    # Config refuses what it can see before a launch
    for call in (lambda: con.rank_candidates([E], [0], [0], [1], None), lambda: con.rank_candidates([0], [1], [0]),
                 lambda: con.rank_candidates(hh, tt, rr, tails, heads[:, :5]), lambda: con.rank_candidates(hh, tt, rr, tails[:5], None),
                 lambda: con.rank_candidates(hh, tt, rr, tails.astype(np.float32), None), lambda: con.rank_triples_sampled([0], [-1], [0], 5),
                 lambda: con.rank_triples_sampled(hh, tt, rr, -1), lambda: con.validation_link_prediction(candidates=-1)):
        with pytest.raises(pkg.KgeError):
            call()
    # FILTERED before importTestFiles (a failed import leaves the library without evaluation lists); unfiltered still ranks
    nothing = tmp_path / "train_only"
    os.makedirs(str(nothing))
    L.setInPath((str(nothing) + "/").encode())
    L.kge_clear_error()
    L.importTestFiles()
    L.kge_clear_error()
    assert raw_call(con, h, t, r, n, dt_, C, dh_, C, C, FILTERED, 0, counts) == KGE_ERR_NO_DATASET and untouched()
    assert raw_call(con, h, t, r, n, None, 0, None, 0, C, DRAWN | TYPED, 0, counts) == KGE_ERR_NO_DATASET and untouched()
    L.kge_clear_error()
    assert raw_call(con, h, t, r, n, dt_, C, dh_, C, C, 0, 0, counts) == 0
    got = counts.cpu().numpy()
    assert np.array_equal(got[:, :, 0], base[:, :, 0]) and np.array_equal(got[:, :, 1], base[:, :, 0])


def test_transr_relation_dimension_above_1024_is_unsupported():
    import torch
    case = case_of("transr", 8, 8, "random")
    con = engine_for(case, "transr", 8, 8)
    z = torch.zeros(2, dtype=torch.int32, device=con.device)
    counts = torch.full((2, 2, 2), -9, dtype=torch.int64, device=con.device)
    assert raw_call(con, z, z, z, 2, None, 0, None, 0, 4, DRAWN, 0, counts, desc=con._desc_with(rel_dim=1025)) == KGE_ERR_UNSUPPORTED
    assert bool((counts == -9).all().item())
    con.lib.kge_clear_error()
