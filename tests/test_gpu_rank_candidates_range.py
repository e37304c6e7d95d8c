"""kge_rank_candidates_range through the C interface, one process: the SUM of its counts over any cut of [0, E) into row ranges
equals kge_rank_candidates on the whole table, element for element -- supplied lists (per triple, shared, one side only, with
pads, ids past the table, repeats, the target and the fixed entity), drawn lists (plain, typed, tail only), filtered or not, at
every rung of the team-shape ladder, list lengths around one batch of ids, and with the list cut into slices (64-bit atomics).
A disabled triple keeps zero counts in every range; every element of the output is written; the refusals write nothing."""
import ctypes

import numpy as np
import pytest

from shard_rig import make_config
from test_gpu_lp_shard import known_set, read_triples

pytestmark = pytest.mark.gpu

KGE_ERR_NO_DATASET, KGE_ERR_BAD_ARG, KGE_ERR_UNSUPPORTED = -2, -3, -4
FILTERED, DRAWN, TYPED, NO_HEAD = 1, 2, 4, 8
LANES = {7: 16, 24: 16, 48: 16, 100: 32, 200: 64, 300: 64, 520: 64}      # dimension -> L, one per rung of for_team_shape
CASES = [(d, c) for d, L in LANES.items() for c in (1, 3, L - 1, L, L + 1, 2 * L + 5)]
CONFIGS = {}


@pytest.fixture(scope="module")
def typed_graph(tmp_path_factory):
    from openkeonspark_amd import synthetic
    return synthetic.make_typed_dataset(str(tmp_path_factory.mktemp("cand_range") / "kg1003"), synthetic.SMALL_TYPED, entities=1003,
                                        train=6000, valid=100, test=60)


def config(path, dim):
    """One TransE config per dimension (tables scaled by 3), kept for the module: the library holds `path`'s evaluation files."""
    from openkeonspark_amd import _lib
    assert hasattr(_lib.lib(), "kge_rank_candidates_range"), "kge_rank_candidates_range is not exported"
    if dim not in CONFIGS:
        CONFIGS[dim] = make_config(dim, path=path)
    return CONFIGS[dim]


def cuts(E):
    chunk = -(-E // 8)
    return {"one": [(0, E)], "first_row": [(0, 1), (1, E)], "empty_middle": [(0, 137), (137, 137), (137, E)],
            "eight": [(g * chunk, min((g + 1) * chunk, E)) for g in range(8)]}


def triples_of(path, E):
    """The validation triples, five test triples and one disabled triple (h = E): int64 [n, 3] (h, t, r)."""
    va, te = np.stack(read_triples(path, "valid2id.txt"), axis=1), np.stack(read_triples(path, "test2id.txt"), axis=1)
    tr = np.concatenate([va, te[:5], va[:1]])
    tr[-1, 0] = E
    return tr


def supplied_lists(con, path, tr, C, seed):
    """Per-triple lists int32 [n, C] for both sides: random ids, and at one place of every list (six places where C >= 8) a
    -1 pad, an id >= E, a repeat of the list's first id, the target, the fixed entity, or the known tail / head of the
    request that scores lowest (fp64) -- that one is below the true triple for many requests, so the filter has work."""
    E = con.entTotal
    rng = np.random.default_rng(seed)
    params = con.get_parameters()
    norm = lambda x: x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12))
    en, rn = norm(params["ent_embeddings"].astype(np.float64)), norm(params["rel_embeddings"].astype(np.float64))
    known_tails, known_heads = {}, {}
    for h, t, r in known_set(path):
        known_tails.setdefault((h, r), []).append(t)
        known_heads.setdefault((t, r), []).append(h)
    lists = rng.integers(0, E, (2, len(tr), C))
    for i, (h, t, r) in enumerate(tr.tolist()):
        if h >= E:
            continue
        for side in (0, 1):
            fixed, target = (t, h) if side else (h, t)
            others = [x for x in (known_heads.get((t, r), []) if side else known_tails.get((h, r), [])) if x != target]
            if others:
                sc = np.abs(en[others] + rn[r] - en[t]).sum(1) if side else np.abs(en[h] + rn[r] - en[others]).sum(1)
                best_known = others[int(np.argmin(sc))]
            else:
                best_known = int(rng.integers(0, E))
            for q in range(1 if C < 8 else 6):
                kind, pos = (i + q + side) % 6, (7 * i + 3 * q) % C
                lists[side, i, pos] = (-1, E + (i % 3) * 1000, lists[side, i, 0], target, fixed, best_known)[kind]
    return lists.astype(np.int32)


def run_cut(con, parts, ids, query, tail, head, C, flags, seed):
    """kge_rank_candidates_range over every range of `parts`, each on a tensor of its own rows and into a buffer pre-filled
    with -9 -> (the per-range counts [len(parts), n, 2, 2] on the device, whether every element was written)."""
    import torch
    from openkeonspark_amd import _lib
    ent, rel = con._tables[0], con._tables[1]
    n = ids.shape[1]
    per_range, written = [], torch.ones((), dtype=torch.bool, device=con.device)
    ptr = lambda x: None if x is None else x[0].data_ptr()
    stride = lambda x: 0 if x is None else x[1]
    for lo, hi in parts:
        part = ent[lo:hi].clone() if hi > lo else torch.zeros((1, ent.shape[1]), dtype=ent.dtype, device=ent.device)
        c = torch.full((n, 2, 2), -9, dtype=torch.int64, device=con.device)
        rc = con.lib.kge_rank_candidates_range(ctypes.byref(con._desc), _lib.table_ptrs([part.data_ptr(), rel.data_ptr()]), lo, hi - lo,
                                               query.data_ptr(), ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n,
                                               ptr(tail), stride(tail), ptr(head), stride(head), C, flags, seed, c.data_ptr(), con._stream())
        _lib.check(rc, con.lib)
        written &= (c >= 0).all()
        per_range.append(c)
    return torch.stack(per_range), written


def whole_table(con, ids, tail, head, C, flags, seed):
    import torch
    from openkeonspark_amd import _lib
    n = ids.shape[1]
    c = torch.full((n, 2, 2), -9, dtype=torch.int64, device=con.device)
    ptr = lambda x: None if x is None else x[0].data_ptr()
    stride = lambda x: 0 if x is None else x[1]
    rc = con.lib.kge_rank_candidates(ctypes.byref(con._desc), con._tab_ptrs, ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n,
                                     ptr(tail), stride(tail), ptr(head), stride(head), C, flags, seed, c.data_ptr(), con._stream())
    _lib.check(rc, con.lib)
    return c.cpu().numpy()


def device_inputs(con, tr):
    """-> (ids int32 device [3, n], the raw h and t rows [n][2][D]; the disabled triple's rows are never read)."""
    import torch
    ids = torch.from_numpy(np.ascontiguousarray(tr.T.astype(np.int32))).to(con.device)
    inside = ids[:2].t().reshape(-1).long().clamp(0, con.entTotal - 1)
    return ids, con._tables[0].index_select(0, inside).contiguous()


@pytest.mark.parametrize("slices", [0, 3])
@pytest.mark.parametrize("dim,C", CASES)
def test_the_sum_over_any_cut_is_the_whole_table(typed_graph, dim, C, slices):
    import torch
    con = config(typed_graph, dim)
    E = con.entTotal
    assert E == 1003
    tr = triples_of(typed_graph, E)
    n = len(tr)
    ids, query = device_inputs(con, tr)
    own = supplied_lists(con, typed_graph, tr, C, seed=dim * 1000 + C)
    skipped = (own < 0) | (own >= E)
    assert skipped.any() and (own == tr[:, 1][None, :, None])[0].any() and (own == tr[:, 0][None, :, None])[0].any()
    stride = C + 3                                                   # lists with a gap between them
    padded = np.full((2, n, stride), 5, dtype=np.int32)
    padded[:, :, :C] = own
    dev = torch.from_numpy(padded).to(con.device)
    per_tail, per_head = (dev[0], stride), (dev[1], stride)
    shared = (torch.from_numpy(np.ascontiguousarray(own[0, 3])).to(con.device), 0)
    modes = {"lists": (per_tail, per_head, FILTERED, 0), "lists_raw": (per_tail, per_head, 0, 0),
             "shared": (shared, shared, FILTERED, 0), "tail_only": (per_tail, None, FILTERED, 0), "head_shared": (None, shared, 0, 0),
             "drawn": (None, None, DRAWN | FILTERED, 11), "drawn_raw": (None, None, DRAWN, 2 ** 64 - 3),
             "drawn_typed": (None, None, DRAWN | TYPED | FILTERED, 5), "drawn_tail": (None, None, DRAWN | NO_HEAD | FILTERED, 11)}
    assert con.lib.kge_set_option(b"rankc_slices", slices) == 0
    try:
        want = {k: whole_table(con, ids, *m[:2], C, *m[2:]) for k, m in modes.items()}
        # nothing below passes vacuously: the reference counts something, filters something, and the sides differ
        for k in ("lists", "drawn"):
            w = want[k]
            assert (w[:, :, 0] > 0).any() and (w[:, 0] != w[:, 1]).any(), k
        assert (want["lists"][:, :, 1] < want["lists"][:, :, 0]).any()      # (the lists hold known entities on purpose)
        assert not any(w[-1].any() for w in want.values())           # the disabled triple
        assert not want["tail_only"][:, 1].any() and not want["head_shared"][:, 0].any() and not want["drawn_tail"][:, 1].any()
        assert np.array_equal(want["lists_raw"][:, :, 1], want["lists"][:, :, 0])
        results = {(k, name): run_cut(con, parts, ids, query, *m[:2], C, *m[2:]) for k, m in modes.items()
                   for name, parts in cuts(E).items()}
        for (k, name), (per_range, written) in results.items():
            got = per_range.cpu().numpy()
            assert bool(written.item()), (k, name)
            assert not got[:, -1].any(), (k, name)                   # disabled: zero in every range
            assert np.array_equal(got.sum(0), want[k]), (k, name)
            if name == "empty_middle":
                assert not got[1].any()
            if name == "eight" and k == "lists":
                assert got.reshape(8, -1).any(axis=1).all()          # every range contributes
    finally:
        con.lib.kge_set_option(b"rankc_slices", 0)


def test_refusals_write_nothing(typed_graph, tmp_path):
    import os
    import torch
    from openkeonspark_amd import _lib
    con = config(typed_graph, 24)
    L, E = con.lib, con.entTotal
    tr = triples_of(typed_graph, E)[:12]
    n, C = len(tr), 9
    ids, query = device_inputs(con, tr)
    h, t, r = ids[0], ids[1], ids[2]
    lists = torch.from_numpy(supplied_lists(con, typed_graph, tr, C, 4)).to(con.device)
    dt_, dh_ = lists[0], lists[1]
    counts = torch.full((n, 2, 2), -9, dtype=torch.int64, device=con.device)
    untouched = lambda: bool((counts == -9).all().item())
    ptr = lambda x: None if x is None else x.data_ptr()

    def call(h=h, t=t, r=r, n=n, tail=dt_, ts=C, head=dh_, hs=C, C=C, flags=FILTERED, lo=0, rows=E, query=query, counts=counts, desc=None,
             tabs=None):
        rc = L.kge_rank_candidates_range(ctypes.byref(desc if desc is not None else con._desc), tabs if tabs is not None else con._tab_ptrs,
                                         lo, rows, ptr(query), ptr(h), ptr(t), ptr(r), n, ptr(tail), ts, ptr(head), hs, C, flags, 0,
                                         ptr(counts), con._stream())
        torch.cuda.synchronize()
        return rc
    good = whole_table(con, ids, (dt_, C), (dh_, C), C, FILTERED, 0)
    assert call() == 0 and np.array_equal(counts.cpu().numpy(), good) and good.any()
    counts.fill_(-9)
    for model in (1, 2, 3):                                           # TransH, TransR, TransD
        assert call(desc=con._desc_with(model=model)) == KGE_ERR_UNSUPPORTED and untouched()
    assert call(desc=con._desc_with(ent_dim=1025)) == KGE_ERR_UNSUPPORTED and untouched()
    for lo, rows in ((1, E), (-1, 2), (0, -1), (E + 1, 0), (0, E + 1)):       # a range outside the table
        assert call(lo=lo, rows=rows) == KGE_ERR_BAD_ARG and untouched(), (lo, rows)
    assert call(query=None) == KGE_ERR_BAD_ARG and untouched()
    # what kge_rank_candidates refuses
    bad = [dict(h=None), dict(t=None), dict(r=None), dict(n=-1), dict(n=1 << 30), dict(C=-1), dict(C=1 << 31),
           dict(tail=None, head=None),                                # no list and no DRAWN
           dict(head=None, flags=FILTERED | DRAWN),                   # a list with DRAWN
           dict(flags=FILTERED | TYPED), dict(flags=NO_HEAD),         # TYPED / NO_HEAD without DRAWN
           dict(ts=C - 1), dict(hs=C - 1),                            # a stride shorter than the list
           dict(flags=16),                                            # an unknown flag
           dict(h=None, n=0),                                         # null pointers are refused with n == 0 too
           dict(tabs=_lib.table_ptrs([con._tables[0].data_ptr(), None]))]
    for kw in bad:
        assert call(**kw) == KGE_ERR_BAD_ARG and untouched(), sorted(kw)
    assert call(counts=None) == KGE_ERR_BAD_ARG
    L.kge_clear_error()
    # n == 0 writes nothing (and needs no query rows); n_cand == 0 and rows == 0 only zero
    assert call(n=0, query=None) == 0 and untouched()
    assert call(C=0, ts=0, hs=0) == 0 and not counts.any().item()
    counts.fill_(-9)
    assert call(rows=0) == 0 and not counts.any().item()
    counts.fill_(-9)
    assert call(lo=E, rows=0) == 0 and not counts.any().item()
    counts.fill_(-9)
    assert call() == 0 and np.array_equal(counts.cpu().numpy(), good)         # a later call still works
    # FILTERED / TYPED before importTestFiles (a failed import leaves the library without evaluation lists); unfiltered still ranks
    nothing = tmp_path / "train_only"
    os.makedirs(str(nothing))
    L.setInPath((str(nothing) + "/").encode())
    L.kge_clear_error()
    L.importTestFiles()
    L.kge_clear_error()
    counts.fill_(-9)
    assert call() == KGE_ERR_NO_DATASET and untouched()
    assert call(n=0) == KGE_ERR_NO_DATASET and untouched()
    assert call(tail=None, head=None, flags=DRAWN | TYPED) == KGE_ERR_NO_DATASET and untouched()
    L.kge_clear_error()
    assert call(flags=0) == 0
    got = counts.cpu().numpy()
    assert np.array_equal(got[:, :, 0], good[:, :, 0]) and np.array_equal(got[:, :, 1], good[:, :, 0])
    L.setInPath((typed_graph + "/").encode())
    con.init_link_prediction()
    assert call() == 0 and np.array_equal(counts.cpu().numpy(), good)
