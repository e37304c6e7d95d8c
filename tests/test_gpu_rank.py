"""kge_rank_triples / Config.rank_triples / Config.validation_link_prediction: filtered ranks of caller-supplied triples from the
fused candidate-major kernel (csrc/rank.hip).  Every comparison is an exact integer equality: against the existing ranker
(link_prediction's columns 0..3 over the whole test set) and against the definition computed in numpy from test_step's scores
(which test_relation_grouped_ranker_equals_generic_predict_path pins as the ranker's bits), a Python set of the known triples
and the type lists of type_constrain.txt."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from openkeonspark_amd import _lib

pytestmark = pytest.mark.gpu

KGE_ERR_NO_DATASET, KGE_ERR_BAD_ARG, KGE_ERR_UNSUPPORTED = -2, -3, -4
MODELS = ["TransE", "TransH", "TransD", "TransR"]


def make_config(kg, model="TransE", dim=40, ent_dim=0, rel_dim=0):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(os.path.join(GOLDEN, kg))
    con.set_work_threads(1)
    con.set_dimension(dim)
    if ent_dim:
        con.set_ent_dimension(ent_dim)
        con.set_rel_dimension(rel_dim)
    con.set_test_link_prediction(True)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    for t in con._tables:                       # spread the scores: xavier-initialised tables rank almost at random
        t.mul_(3.0)
    con.tables_changed()
    return con


def split(kg, name):
    """The triples of a split file as int64 [n, 3] (h, t, r), file order."""
    with open(os.path.join(GOLDEN, kg, name + "2id.txt")) as f:
        tok = f.read().split()
    n = int(tok[0])
    return np.asarray(tok[1:1 + 3 * n], dtype=np.int64).reshape(n, 3)


def lp_order(kg):
    """The test triples in link_prediction's order: sorted by (r, h, t)."""
    a = split(kg, "test")
    return a[np.lexsort((a[:, 1], a[:, 0], a[:, 2]))]


class Definition:
    """The four counts from their definition, in numpy; one test_step call per (triple, side), cached per (side, fixed, r)."""

    def __init__(self, kg):
        self.known_tails, self.known_heads = {}, {}
        for name in ("train", "valid", "test"):
            for h, t, r in split(kg, name).tolist():
                self.known_tails.setdefault((h, r), set()).add(t)
                self.known_heads.setdefault((t, r), set()).add(h)
        with open(os.path.join(GOLDEN, kg, "type_constrain.txt")) as f:
            tok = [int(x) for x in f.read().split()]
        self.types = {}                           # (relation, side) -> ids; per relation the head list, then the tail list
        p, seen = 1, {}
        while p + 1 < len(tok):
            rel, tot = tok[p], tok[p + 1]
            side = 1 if rel not in seen else 0    # first line of a relation: heads (side 1), second: tails (side 0)
            seen[rel] = True
            self.types[(rel, side)] = tok[p + 2:p + 2 + tot]
            p += 2 + tot

    def counts(self, con, triples, test_head=True):
        E = con.entTotal
        ar = np.arange(E)
        out = np.zeros((len(triples), 2, 4), dtype=np.int64)
        cache = {}
        for i, (h, t, r) in enumerate(np.asarray(triples).tolist()):
            for side in ((0, 1) if test_head else (0,)):
                fixed, target = (t, h) if side else (h, t)
                key = (side, fixed, r)
                if key not in cache:
                    rr = np.full(E, r)
                    s = con.test_step(ar, np.full(E, t), rr) if side else con.test_step(np.full(E, h), ar, rr)
                    known = np.zeros(E, dtype=bool)
                    known[list((self.known_heads if side else self.known_tails).get((fixed, r), ()))] = True
                    typed = np.zeros(E, dtype=bool)
                    typed[self.types.get((r, side), [])] = True
                    cache[key] = (np.asarray(s).reshape(-1).copy(), known, typed)
                s, known, typed = cache[key]
                with np.errstate(invalid="ignore"):
                    below = s < s[target]          # NaN never counts: the reference's `<`
                below[target] = False
                out[i, side] = [below.sum(), (below & ~known).sum(), (below & typed).sum(), (below & typed & ~known).sum()]
        return out


@pytest.fixture(scope="module")
def definition():
    return Definition("kg_small")


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("test_head", [True, False])
def test_equals_the_existing_ranker_on_the_whole_test_set(model, test_head):
    con = make_config("kg_small", model)
    tt = lp_order("kg_small")
    want, want_metrics = con.link_prediction(test_head=test_head)
    got, metrics = con.rank_triples(tt[:, 0], tt[:, 1], tt[:, 2], test_head=test_head)
    assert got.dtype == np.int64 and got.shape == (len(tt), 2, 4)
    assert np.array_equal(got, want[:, :, :4])
    assert got[:, 0, 0].any()
    if not test_head:
        assert not got[:, 1].any()
    assert metrics == want_metrics


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_any_order_mixed_relations_and_repeats(model):
    con = make_config("kg_small", model)
    tt, va = lp_order("kg_small"), split("kg_small", "valid")
    base_t, _ = con.rank_triples(tt[:, 0], tt[:, 1], tt[:, 2])
    base_v, _ = con.rank_triples(va[:, 0], va[:, 1], va[:, 2])
    pool = np.concatenate([tt, va])
    want = np.concatenate([base_t, base_v])
    rng = np.random.default_rng(11)
    pick = np.concatenate([rng.permutation(len(pool)), rng.integers(0, len(pool), 25)])   # everything once, 25 repeats
    rng.shuffle(pick)
    got, _ = con.rank_triples(pool[pick, 0], pool[pick, 1], pool[pick, 2])
    assert np.array_equal(got, want[pick])


# 3 ------------------------------------------------------------------------------------------------------------------------
def made_up_triples(definition, E, R, rng):
    """20 triples in no split: one whose (h, r) has no known tail, one with h == t."""
    all_known = {(h, t, r) for (h, r), ts in definition.known_tails.items() for t in ts}
    out = []
    h = next(h for h in range(E) if (h, 0) not in definition.known_tails)
    out.append((h, (h + 7) % E, 0))                     # (h, r) without any known tail
    out.append((5, 5, 3))                               # h == t
    while len(out) < 20:
        c = (int(rng.integers(E)), int(rng.integers(E)), int(rng.integers(R)))
        if c not in all_known:
            out.append(c)
    assert not any(c in all_known for c in out)
    return np.asarray(out, dtype=np.int64)


@pytest.mark.parametrize("model", MODELS)
def test_equals_the_definition(model, definition):
    con = make_config("kg_small", model)
    rng = np.random.default_rng(5)
    train = split("kg_small", "train")
    triples = np.concatenate([split("kg_small", "valid"), train[rng.choice(len(train), 500, replace=False)],
                              made_up_triples(definition, con.entTotal, con.relTotal, rng)])
    assert np.bincount(triples[:, 2]).max() > 64          # a relation with far more requests than one block holds
    got, _ = con.rank_triples(triples[:, 0], triples[:, 1], triples[:, 2])
    want = definition.counts(con, triples)
    assert np.array_equal(got, want)
    assert (got[:, :, 1] < got[:, :, 0]).any() and (got[:, :, 2] < got[:, :, 0]).any()   # the filter and the type lists bite


# 4 ------------------------------------------------------------------------------------------------------------------------
LADDER = [("TransE", d, 0, 0) for d in (7, 24, 64, 100, 200, 260, 520)] + [("TransD", d, 0, 0) for d in (7, 24, 64, 100, 200, 260, 520)] + \
         [("TransR", 8, 8, 24), ("TransR", 8, 8, 260)]


@pytest.mark.parametrize("model,dim,ent_dim,rel_dim", LADDER)
def test_every_rung_of_the_ladder(model, dim, ent_dim, rel_dim, definition):
    con = make_config("kg_small", model, dim, ent_dim, rel_dim)
    triples = np.concatenate([split("kg_small", "valid"), split("kg_small", "test")])
    got, _ = con.rank_triples(triples[:, 0], triples[:, 1], triples[:, 2])
    assert np.array_equal(got, definition.counts(con, triples))
    assert got[:, :, 0].any()


@pytest.mark.parametrize("model,dim", [("TransE", 40), ("TransE", 100), ("TransE", 200), ("TransH", 40), ("TransH", 200), ("TransD", 200)])
def test_candidates_within_an_ulp_of_the_true_triple(model, dim):
    """Hundreds of entity rows are copies of a test triple's tail row and of its head row with single elements moved by one
    ulp, so their scores lie within a few ulps of the true triple's, on either side or tied: a count then depends on the last
    bit of every score, and the counts of the whole test set must still equal link_prediction's.  (The relation vector's
    product rn = raw * inv is contracted into the tail side's hn + rn in lp_score_kernel and not on the head side; a ranker
    that rounds it otherwise differs here.)"""
    import torch
    con = make_config("kg_small", model, dim)
    tt = lp_order("kg_small")
    rng = np.random.default_rng(17)
    used = set(tt[:, 0].tolist()) | set(tt[:, 1].tolist())
    free = np.array([e for e in range(con.entTotal) if e not in used])
    rng.shuffle(free)
    ent = con._tables[0].cpu().numpy().copy()
    per = len(free) // 8
    for k, i in enumerate(rng.choice(len(tt), 4, replace=False)):      # four triples: copies of the tail row, copies of the head row
        for side, src in enumerate((tt[i, 1], tt[i, 0])):
            rows = free[(2 * k + side) * per:(2 * k + side + 1) * per]
            block = np.repeat(ent[src][None, :], len(rows), axis=0)
            for j in range(len(rows)):
                cols = rng.choice(block.shape[1], rng.integers(0, 4), replace=False)       # 0 .. 3 elements, one ulp up or down
                block[j, cols] = np.nextafter(block[j, cols], np.where(rng.random(len(cols)) < 0.5, np.float32(-np.inf), np.float32(np.inf)).astype(np.float32))
            ent[rows] = block
    con._tables[0].copy_(torch.from_numpy(ent).to(con.device))
    con.tables_changed()
    want = con.link_prediction()[0][:, :, :4]
    got, _ = con.rank_triples(tt[:, 0], tt[:, 1], tt[:, 2])
    assert np.array_equal(got, want)


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kg,slices", [("kg_small", (1, 3, 7)), ("kg_tiny", (64,))])
def test_counts_do_not_depend_on_the_slices(kg, slices):
    L = _lib.lib()
    for model in ("TransE", "TransH"):
        con = make_config(kg, model)
        triples = np.concatenate([split(kg, "valid"), split(kg, "test")])
        auto, _ = con.rank_triples(triples[:, 0], triples[:, 1], triples[:, 2])
        assert auto[:, :, 0].any()
        try:
            for n in slices:
                assert L.kge_set_option(b"rank_slices", n) == 0
                got, _ = con.rank_triples(triples[:, 0], triples[:, 1], triples[:, 2])
                assert np.array_equal(got, auto), (model, n)
        finally:
            L.kge_set_option(b"rank_slices", 0)


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_edges(definition):
    con = make_config("kg_small", "TransE")
    va, tt = split("kg_small", "valid"), lp_order("kg_small")
    lp_before = con.link_prediction()[0]
    one, met = con.rank_triples(va[:1, 0], va[:1, 1], va[:1, 2])                       # n = 1
    assert one.shape == (1, 2, 4) and np.array_equal(one, definition.counts(con, va[:1]))
    none, met0 = con.rank_triples([], [], [])                                          # n = 0
    assert none.shape == (0, 2, 4) and none.dtype == np.int64 and set(met0) == set(met)
    # two calls in a row on different sets, a link_prediction() in between: no stale counts or workspace state
    a, _ = con.rank_triples(va[:, 0], va[:, 1], va[:, 2])
    assert np.array_equal(con.link_prediction()[0], lp_before)
    b, _ = con.rank_triples(tt[:, 0], tt[:, 1], tt[:, 2])
    assert np.array_equal(a, definition.counts(con, va)) and np.array_equal(b, lp_before[:, :, :4])
    assert np.array_equal(con.rank_triples(va[:, 0], va[:, 1], va[:, 2])[0], a)


@pytest.mark.parametrize("model", ["TransE", "TransD"])
def test_nan_row_as_candidate_and_as_target(model, definition):
    con = make_config("kg_small", model)
    va = split("kg_small", "valid")
    bad = int(va[0, 1])                         # the tail of the first validation triple: a target there, a candidate elsewhere
    con._tables[0][bad] = float("nan")
    con.tables_changed()
    got, _ = con.rank_triples(va[:, 0], va[:, 1], va[:, 2])
    want = definition.counts(con, va)
    assert not want[0, 0].any()                 # NaN target: nothing scores below it
    assert want[1:, :, 0].any()
    assert np.array_equal(got, want)


# 7 ------------------------------------------------------------------------------------------------------------------------
def raw_call(con, L, h, t, r, n, counts, desc=None, test_head=1):
    ptr = lambda x: None if x is None else x.data_ptr()
    rc = L.kge_rank_triples(ctypes.byref(desc if desc is not None else con._desc), con._tab_ptrs, ptr(h), ptr(t), ptr(r), n, test_head,
                            ptr(counts), con._stream())
    import torch
    torch.cuda.synchronize()
    return rc


def test_errors_leave_the_counts_untouched(tmp_path, monkeypatch):
    import torch
    import openkeonspark_amd as pkg
    con = make_config("kg_small", "TransE", dim=16)
    L = con.lib
    va = split("kg_small", "valid")
    n = len(va)
    h, t, r = (torch.from_numpy(va[:, i].astype(np.int32)).to(con.device) for i in range(3))
    counts = torch.full((n, 2, 4), -9, dtype=torch.int64, device=con.device)
    untouched = lambda: bool((counts == -9).all().item())
    assert raw_call(con, L, None, t, r, n, counts) == KGE_ERR_BAD_ARG and untouched()
    assert raw_call(con, L, h, None, r, n, counts) == KGE_ERR_BAD_ARG and untouched()
    assert raw_call(con, L, h, t, None, n, counts) == KGE_ERR_BAD_ARG and untouched()
    assert raw_call(con, L, h, t, r, n, None) == KGE_ERR_BAD_ARG
    assert raw_call(con, L, h, t, r, -1, counts) == KGE_ERR_BAD_ARG and untouched()
    assert raw_call(con, L, h, t, r, n, counts, desc=con._desc_with(ent_dim=1025)) == KGE_ERR_UNSUPPORTED and untouched()
    assert raw_call(con, L, h, t, r, 0, counts) == 0 and untouched()                 # n == 0: arguments and files only
    assert raw_call(con, L, None, t, r, 0, counts) == KGE_ERR_BAD_ARG and raw_call(con, L, h, t, r, 0, None) == KGE_ERR_BAD_ARG
    L.kge_clear_error()
    # an id out of range: KgeError on the host, nothing launched
    launched = []
    monkeypatch.setattr(pkg.rank_eval, "rank_device", lambda *a: launched.append(a))
    for bad in (([con.entTotal], [0], [0]), ([0], [-1], [0]), ([0], [1], [con.relTotal])):
        with pytest.raises(pkg.KgeError):
            con.rank_triples(*bad)
    assert not launched
    monkeypatch.undo()
    # before importTestFiles (a failed import leaves the library without evaluation lists)
    empty = tmp_path / "train_only"
    os.makedirs(str(empty))
    L.setInPath((str(empty) + "/").encode())
    L.kge_clear_error()
    L.importTestFiles()
    L.kge_clear_error()
    assert raw_call(con, L, h, t, r, n, counts) == KGE_ERR_NO_DATASET and untouched()
    assert raw_call(con, L, h, t, r, 0, counts) == KGE_ERR_NO_DATASET and untouched()
    L.kge_clear_error()
    # and with the files back the same buffers are ranked
    L.setInPath((os.path.join(GOLDEN, "kg_small") + "/").encode())
    con.init_link_prediction()
    assert raw_call(con, L, h, t, r, n, counts) == 0
    assert np.array_equal(counts.cpu().numpy(), con.rank_triples(va[:, 0], va[:, 1], va[:, 2])[0])


def test_transr_relation_dimension_above_1024_is_unsupported():
    import torch
    con = make_config("kg_tiny", "TransR", dim=8, ent_dim=8, rel_dim=8)
    z = torch.zeros(2, dtype=torch.int32, device=con.device)
    counts = torch.full((2, 2, 4), -9, dtype=torch.int64, device=con.device)
    assert raw_call(con, con.lib, z, z, z, 2, counts, desc=con._desc_with(rel_dim=1025)) == KGE_ERR_UNSUPPORTED
    assert bool((counts == -9).all().item())
    con.lib.kge_clear_error()


def _sharded_worker(rank, world, port, out_dir, data):
    import openkeonspark_amd as pkg
    from shard_rig import finish_rank, start_rank
    import datetime
    con = start_rank(rank, world, port, data, timeout=datetime.timedelta(seconds=60))
    refused = []
    for call in (lambda: con.rank_triples([0], [1], [0]), lambda: con.validation_link_prediction()):
        try:
            call()
            refused.append(0)
        except pkg.KgeError:
            refused.append(1)
    finish_rank(con, out_dir, world, rank, refused=np.array(refused))


def test_a_sharded_entity_table_is_refused(tmp_path):
    import torch.multiprocessing as mp
    from shard_rig import KG, load_ranks
    mp.start_processes(_sharded_worker, args=(2, 37100 + os.getpid() % 1000, str(tmp_path), KG), nprocs=2, join=True, start_method="spawn")
    for z in load_ranks(str(tmp_path), 2):
        assert z["refused"].tolist() == [1, 1]


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_validation_link_prediction(monkeypatch):
    con = make_config("kg_small", "TransH")
    L = con.lib
    va = split("kg_small", "valid")
    V = len(va)
    want, want_metrics = con.rank_triples(va[:, 0], va[:, 1], va[:, 2])
    got, metrics = con.validation_link_prediction()
    assert np.array_equal(got, want) and metrics == want_metrics
    tail_only, m_tail = con.validation_link_prediction(test_head=False)
    assert np.array_equal(tail_only[:, 0], want[:, 0]) and not tail_only[:, 1].any() and "l_filter_tot" not in m_tail
    idx = (np.arange(7) * V) // 7
    s7, m7 = con.validation_link_prediction(sample=7)
    assert s7.shape == (7, 2, 4) and np.array_equal(s7, want[idx])
    assert m7 == con.rank_triples(va[idx, 0], va[idx, 1], va[idx, 2])[1]
    # the device ids are kept between calls
    import torch
    uploads = []
    real = torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: (uploads.append(1), real(a))[1])
    again, _ = con.validation_link_prediction(sample=7)
    monkeypatch.undo()
    assert np.array_equal(again, s7) and not uploads
    assert np.array_equal(con.validation_link_prediction()[0], want)

    # the libc rand() stream is unmoved: getValidBatch draws the negatives of a fresh run
    def draw():
        arrs = [np.zeros(V, np.int64) for _ in range(6)]
        L.getValidBatch(*[a.ctypes.data for a in arrs])
        _lib.raise_if_error(L)
        return arrs
    con.init_valid_triple_classification()
    L.kge_set_option(b"libc_rand_restart", 1)
    fresh = draw()
    L.kge_set_option(b"libc_rand_restart", 1)
    con.validation_link_prediction()
    con.validation_link_prediction(sample=5)
    after = draw()
    for a, b in zip(fresh, after):
        assert np.array_equal(a, b)
    assert not np.array_equal(fresh[4], draw()[4])         # (a second draw does move on: the comparison can fail)
