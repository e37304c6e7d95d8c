"""Top-k entity prediction over a row range of the entity table (kge_topk_entities_range + kge_topk_merge_keys) and the
shard-aware Config.top_k_tails / top_k_heads built on them: the whole table as one range against kge_topk_entities bit for bit
(every dimension bucket, both candidate paths), bit-exact invariance under any cut of the table (empty, one-row and
under-filled ranges; unfiltered, filtered, typed, both), the model refusal, 2 and 4 gloo ranks against one process over the
union table, and errors that every rank agrees on.

Every test first checks that the new entry points exist."""
import ctypes
import datetime
import os

import numpy as np
import pytest

from shard_rig import finish_rank, load_ranks, make_config, run_worlds, start_rank, union_config

pytestmark = pytest.mark.gpu
FILTERED, TYPED = 1, 2
UNSUPPORTED = -4


def require_entry_points():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    for name in ("kge_topk_entities_range", "kge_topk_merge_keys"):
        assert hasattr(L, name), name + " is not exported"
    return L


def queries(con, n=48, seed=0):
    """Mixed head / tail queries with repeats; ids at both ends of the table."""
    rng = np.random.default_rng(seed)
    fixed = rng.integers(0, con.entTotal, n)
    rel = rng.integers(0, con.relTotal, n)
    head = rng.integers(0, 2, n).astype(np.int32)
    fixed[:2] = [0, con.entTotal - 1]
    fixed[5:9] = fixed[4]; rel[5:9] = rel[4]; head[5:9] = head[4]
    return fixed, rel, head


def whole_table(con, fixed, rel, head, k, flags=0):
    """kge_topk_entities over the whole table, both sides in one batch."""
    import torch
    from openkeonspark_amd import _lib
    dev, n = con.device, len(fixed)
    f = torch.as_tensor(fixed, dtype=torch.int32, device=dev)
    r = torch.as_tensor(rel, dtype=torch.int32, device=dev)
    h = torch.as_tensor(head, dtype=torch.int32, device=dev)
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    sc = torch.empty((n, k), dtype=torch.float32, device=dev)
    _lib.check(con.lib.kge_topk_entities(ctypes.byref(con._desc), con._tab_ptrs, f.data_ptr(), r.data_ptr(), h.data_ptr(), n, k,
                                         flags, ids.data_ptr(), sc.data_ptr(), con._stream()), con.lib)
    return ids.cpu().numpy(), sc.cpu().numpy()


def ranges_merged(con, parts, fixed, rel, head, k, flags=0):
    """kge_topk_entities_range over each range of the cut `parts` [(lo, hi), ...] -- each range in a tensor of its own, the
    fixed rows passed as query rows -- then kge_topk_merge_keys over the [parts][n][k] key lists.  -> (ids, scores, keys)."""
    import torch
    from openkeonspark_amd import _lib
    L = require_entry_points()
    dev, n, st = con.device, len(fixed), con._stream()
    ent, relt = con._tables[0], con._tables[1]
    f = torch.as_tensor(fixed, dtype=torch.int32, device=dev)
    r = torch.as_tensor(rel, dtype=torch.int32, device=dev)
    h = torch.as_tensor(head, dtype=torch.int32, device=dev)
    qrows = ent.index_select(0, f.long()).contiguous()
    keys = torch.empty((len(parts), n, k), dtype=torch.int64, device=dev)
    for p, (lo, hi) in enumerate(parts):
        part = ent[lo:hi].clone() if hi > lo else torch.empty((1, ent.shape[1]), dtype=ent.dtype, device=dev)
        ptrs = _lib.table_ptrs([part.data_ptr(), relt.data_ptr()])
        _lib.check(L.kge_topk_entities_range(ctypes.byref(con._desc), ptrs, lo, hi - lo, qrows.data_ptr(), f.data_ptr(), r.data_ptr(),
                                             h.data_ptr(), n, k, flags, keys[p].data_ptr(), st), L)
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    sc = torch.empty((n, k), dtype=torch.float32, device=dev)
    _lib.check(L.kge_topk_merge_keys(keys.data_ptr(), n, len(parts), k, ids.data_ptr(), sc.data_ptr(), st), L)
    return ids.cpu().numpy(), sc.cpu().numpy(), keys.cpu().numpy()


def assert_bits(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


# ---------------------------------------------------------------------------------------------------------------------------
# 1-3: one process
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [16, 48, 200, 512, 1024])
def test_whole_table_as_one_range_equals_topk_entities(dim):
    require_entry_points()
    con = make_config(dim)
    E = con.entTotal
    fixed, rel, head = queries(con)
    assert head.any() and not head.all()
    L = con.lib
    for budget in (1 << 30, 0):
        L.kge_set_option(b"topk_table_max_bytes", budget)
        try:
            for k in (1, 10, 1024):
                want = whole_table(con, fixed, rel, head, k)
                ids, sc, keys = ranges_merged(con, [(0, E)], fixed, rel, head, k)
                assert_bits((ids, sc), want, (budget, k))
                assert (ids[:, :min(k, E)] >= 0).all() and (ids[:, E:] == -1).all()
                u = keys[0].view(np.uint64)
                assert (u[:, 1:] >= u[:, :-1]).all()       # each range's list is ascending, padding last
        finally:
            L.kge_set_option(b"topk_table_max_bytes", 1 << 30)


@pytest.fixture(scope="module")
def typed_graph(tmp_path_factory):
    from openkeonspark_amd import synthetic
    return synthetic.make_typed_dataset(str(tmp_path_factory.mktemp("typed_topk")), synthetic.SMALL_TYPED)


def cuts(E):
    return {
        "one": [(0, E)],
        "empty_and_tiny": [(0, 0), (0, 1), (1, 4), (4, 4), (4, E // 2), (E // 2, E)],
        "97_rows": [(lo, min(lo + 97, E)) for lo in range(0, E, 97)],
        "empty_last": [(0, E - 3), (E - 3, E), (E, E)],
    }


@pytest.mark.parametrize("flags", [0, FILTERED, TYPED, FILTERED | TYPED])
def test_any_cut_gives_the_same_bits(typed_graph, flags):
    require_entry_points()
    con = make_config(40, path=typed_graph)
    E = con.entTotal
    fixed, rel, head = queries(con, n=40, seed=flags + 1)
    for k in (10, 100):
        want = whole_table(con, fixed, rel, head, k, flags)
        for name, parts in cuts(E).items():
            ids, sc, keys = ranges_merged(con, parts, fixed, rel, head, k, flags)
            assert_bits((ids, sc), want, (k, name))
            for p, (lo, hi) in enumerate(parts):
                got = keys[p].view(np.uint64)
                real = got != np.uint64(0xFFFFFFFFFFFFFFFF)
                kid = (got & np.uint64(0xFFFFFFFF)).astype(np.int64)
                assert ((kid >= lo) & (kid < hi))[real].all(), (name, p)    # a range offers only its own global ids
                if hi - lo < k:
                    assert (~real[:, hi - lo:]).all(), (name, p)


@pytest.mark.parametrize("model", ["TransH", "TransR", "TransD"])
def test_other_models_are_unsupported(model):
    import torch
    from openkeonspark_amd import _lib
    L = require_entry_points()
    con = make_config(16, model=model, scale=1.0)
    dev, n, k = con.device, 4, 5
    f = torch.zeros(n, dtype=torch.int32, device=dev)
    qrows = torch.zeros((n, 16), dtype=torch.float32, device=dev)
    keys = torch.empty((n, k), dtype=torch.int64, device=dev)
    rc = L.kge_topk_entities_range(ctypes.byref(con._desc), con._tab_ptrs, 0, con.entTotal, qrows.data_ptr(), f.data_ptr(),
                                   f.data_ptr(), f.data_ptr(), n, k, 0, keys.data_ptr(), con._stream())
    assert rc == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------
# 4-5: ranks (gloo, one GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _rank_queries(rank, world, E, R, chunk):
    """Rank g's own queries: ids at every shard boundary, repeats, random ids; the last rank none."""
    if rank == world - 1:
        z = np.zeros(0, dtype=np.int64)
        return z, z
    rng = np.random.default_rng(300 + rank)
    n = 30 + 5 * rank
    f = rng.integers(0, E, n)
    r = rng.integers(0, R, n)
    bounds = sorted({min(g * chunk, E - 1) for g in range(world)} | {min((g + 1) * chunk - 1, E - 1) for g in range(world)})
    f[:len(bounds)] = bounds
    f[len(bounds):2 * len(bounds)] = bounds          # repeated ids
    r[len(bounds):2 * len(bounds)] = r[:len(bounds)]
    return f, r


# (name, side, k, filtered, type_constrained, device inputs, one query per chunk)
CALLS = [("tail", "tail", 10, False, False, False, False),
         ("head_dev", "head", 10, False, False, True, False),
         ("tail_filt", "tail", 25, True, False, False, False),
         ("head_typed_dev", "head", 25, False, True, True, False),
         ("tail_both", "tail", 7, True, True, False, False),
         ("head_1024", "head", 1024, True, False, False, False),
         ("tail_chunked", "tail", 10, True, False, False, True),
         ("head_chunked_dev", "head", 16, False, True, True, True)]


def _rank_worker(rank, world, port, out_dir, data):
    import torch
    import openkeonspark_amd as pkg
    con = start_rank(rank, world, port, data, timeout=datetime.timedelta(seconds=60))
    E, R, chunk = con.entTotal, con.relTotal, con._shard["chunk"]
    f, r = _rank_queries(rank, world, E, R, chunk)
    out = dict(f=f, r=r)
    default_bytes = con.topk_shard_query_bytes
    for name, side, k, filt, typed, on_dev, chunked in CALLS:
        con.topk_shard_query_bytes = 1 if chunked else default_bytes
        a, b = (torch.as_tensor(f, device=con.device), torch.as_tensor(r, device=con.device)) if on_dev else (f, r)
        fn = con.top_k_heads if side == "head" else con.top_k_tails
        ids, sc = fn(a, b, k, filtered=filt, type_constrained=typed)
        if on_dev:
            assert isinstance(ids, torch.Tensor) and ids.device.type != "cpu" and ids.dtype == torch.int64
            ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        else:
            assert isinstance(ids, np.ndarray) and ids.dtype == np.int64 and sc.dtype == np.float32
        out[name + "_ids"], out[name + "_sc"] = ids, sc
    con.topk_shard_query_bytes = default_bytes
    # errors every rank agrees on: an id out of range on rank 0 only, then a different k on every rank
    raised = []
    bad = np.array([E]) if rank == 0 else f
    for fixed, k in ((bad, 5), (f, 5 + rank)):
        try:
            con.top_k_tails(fixed, np.zeros(len(fixed), dtype=np.int64), k)
            raised.append(0)
        except pkg.KgeError:
            raised.append(1)
    out["raised"] = np.array(raised)
    out["after_ids"], out["after_sc"] = con.top_k_tails(f, r, 10)     # a valid call still works afterwards
    refused = 0
    try:
        con.top_k_relations(0, 1, 5)
    except pkg.KgeError:
        refused = 1
    out["refused"] = np.array(refused)
    finish_rank(con, out_dir, world, rank, **out)


@pytest.fixture(scope="module")
def sharded_runs(tmp_path_factory):
    require_entry_points()
    return run_worlds(_rank_worker, tmp_path_factory.mktemp("topk_shard_ranks"), 33900 + os.getpid() % 1000)


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_equal_one_process_over_the_union_table(sharded_runs, world):
    base, data = sharded_runs
    zs = load_ranks(base, world)
    con = union_config(data, zs[0])
    assert con.entTotal == 1003 and con.entTotal % world
    assert len(zs[-1]["f"]) == 0 and len(zs[0]["f"]) > 0
    for g, z in enumerate(zs):
        assert np.array_equal(z["ent"], zs[0]["ent"]) and np.array_equal(z["rel"], zs[0]["rel"])
        for name, side, k, filt, typed, _, _ in CALLS:
            fn = con.top_k_heads if side == "head" else con.top_k_tails
            want = fn(z["f"], z["r"], k, filtered=filt, type_constrained=typed)
            got = (z[name + "_ids"], z[name + "_sc"])
            assert got[0].shape == (len(z["f"]), k), (g, name)
            assert_bits(got, want, (g, name))
        assert_bits((z["after_ids"], z["after_sc"]), (z["tail_ids"], z["tail_sc"]), g)


@pytest.mark.parametrize("world", [2, 4])
def test_bad_calls_raise_on_every_rank(sharded_runs, world):
    base, _ = sharded_runs
    for g, z in enumerate(load_ranks(base, world)):
        assert z["raised"].tolist() == [1, 1], g
        assert int(z["refused"]) == 1, g       # top-k relations still refuse a sharded table
