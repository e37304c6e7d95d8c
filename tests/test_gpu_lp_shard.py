"""Link prediction over a row range of the entity table (kge_link_prediction_range / kge_link_prediction_finish) and the
shard-aware evaluation built on it (Config.link_prediction / link_prediction_distributed / test_step on a table sharded across
ranks): the whole table as one range against kge_link_prediction under a constructive near-tie rule, bit-exact invariance under
any cut of the table, ties with a copied target row, the filtered / typed / ontology columns, 2 and 4 gloo ranks against one
process, sharded test_step, the refusals and the driver's --mode test.

Every test first checks that the new entry points exist: the old ranker is never launched over a shard."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from openkeonspark_amd import rank_eval
from shard_rig import KG, finish_rank, load_ranks, make_config, run_worlds, start_rank, union_config

pytestmark = pytest.mark.gpu
NO_KEY = np.iinfo(np.int64).max


def require_entry_points():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    for name in ("kge_link_prediction_range", "kge_link_prediction_finish", "kge_test_entity_ids"):
        assert hasattr(L, name), name + " is not exported"
    return L


def lp_ranges(con, parts, first=0, count=None, test_head=True):
    """The new entry points over the cut `parts` [(lo, hi), ...] of con's entity table, each range in a tensor of its own:
    -> (out int64 [count, 2, 8], summed counts [count, 2, 4], min keys [count, 2, 4])."""
    import ctypes
    import torch
    from openkeonspark_amd import _lib
    L = require_entry_points()
    if count is None:
        count = con.lib.getTestTotal() - first
    st = con._stream()
    ent, rel = con._tables[0], con._tables[1]
    th = 1 if test_head else 0
    ids = torch.empty(2 * count, dtype=torch.int32, device=con.device)
    _lib.check(L.kge_test_entity_ids(first, count, ids.data_ptr(), st), L)
    query = ent.index_select(0, ids.long()).contiguous()
    tot_c = torch.zeros((count, 2, 4), dtype=torch.int64, device=con.device)
    tot_k = torch.full((count, 2, 4), NO_KEY, dtype=torch.int64, device=con.device)
    for lo, hi in parts:
        part = ent[lo:hi].clone() if hi > lo else torch.empty((1, ent.shape[1]), dtype=ent.dtype, device=ent.device)
        ptrs = _lib.table_ptrs([part.data_ptr(), rel.data_ptr()])
        c = torch.empty_like(tot_c)
        k = torch.empty_like(tot_k)
        _lib.check(L.kge_link_prediction_range(ctypes.byref(con._desc), ptrs, lo, hi - lo, query.data_ptr(), first, count, th,
                                               c.data_ptr(), k.data_ptr(), st), L)
        tot_c += c
        tot_k = torch.minimum(tot_k, k)
    out = np.zeros((count, 2, 8), dtype=np.int64)
    _lib.check(L.kge_link_prediction_finish(first, count, th, tot_c.data_ptr(), tot_k.data_ptr(), out.ctypes.data, st), L)
    return out, tot_c.cpu().numpy(), tot_k.cpu().numpy()


def key_ids(keys):
    return np.where(keys == NO_KEY, -1, (keys & 0xFFFFFFFF).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# host side of the near-tie rule: fp64 scores, the filter and the type lists from the dataset files
# ---------------------------------------------------------------------------------------------------------------------------
def read_triples(path, name):
    a = np.loadtxt(os.path.join(path, name), dtype=np.int64, skiprows=1, ndmin=2)
    return a[:, 0], a[:, 1], a[:, 2]     # h, t, r


def sorted_test_triples(path):
    h, t, r = read_triples(path, "test2id.txt")
    o = np.lexsort((t, h, r))
    return h[o], t[o], r[o]


def known_set(path):
    known = set()
    for name in ("train2id.txt", "valid2id.txt", "test2id.txt"):
        h, t, r = read_triples(path, name)
        known.update(zip(h.tolist(), t.tolist(), r.tolist()))
    return known


def type_lists(path, R):
    heads, tails = [set() for _ in range(R)], [set() for _ in range(R)]
    if not os.path.exists(os.path.join(path, "type_constrain.txt")):
        return heads, tails
    with open(os.path.join(path, "type_constrain.txt")) as f:
        lines = [x for x in f.read().split("\n")[1:] if x.strip()]
    for i in range(0, len(lines) - 1, 2):
        hl, tl = lines[i].split(), lines[i + 1].split()
        heads[int(hl[0])].update(int(x) for x in hl[2:])
        tails[int(tl[0])].update(int(x) for x in tl[2:])
    return heads, tails


def check_near_tie_rule(con, path, out_new, out_old, test_head):
    """Each count of out_new may differ from out_old's only by the number of eligible candidates whose fp64 score lies within a
    few ulp (of the fp32 sums) of the true triple's; the ontology classes must agree wherever the arg-min cannot move (its
    column's counts agree and no eligible candidate is that close to the fp64 minimum or to the true triple)."""
    params = con.get_parameters()
    ent = params["ent_embeddings"].astype(np.float64)
    rel = params["rel_embeddings"].astype(np.float64)
    norm = lambda x: x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12))
    en, rn = norm(ent), norm(rel)
    E = ent.shape[0]
    hs, ts, rs = sorted_test_triples(path)
    known = known_set(path)
    heads, tails = type_lists(path, rel.shape[0])
    ids = np.arange(E)
    flips = 0
    for i in range(len(hs)):
        h, t, r = int(hs[i]), int(ts[i]), int(rs[i])
        for side in ((0, 1) if test_head else (0,)):
            if side == 0:
                sc = np.abs(en[h] + rn[r] - en).sum(1)
                target = t
                kn = np.array([(h, j, r) in known for j in range(E)])
                ty = np.isin(ids, list(tails[r]))
            else:
                sc = np.abs(en + rn[r] - en[t]).sum(1)
                target = h
                kn = np.array([(j, t, r) in known for j in range(E)])
                ty = np.isin(ids, list(heads[r]))
            tol = 64 * np.spacing(np.float32(sc[target]))
            other = ids != target
            near = other & (np.abs(sc - sc[target]) <= tol)
            below = other & (sc < sc[target] + tol)
            cols = [other, other & ~kn, other & ty, other & ty & ~kn]
            key_cols = [other, other if side == 1 else other & ~kn, other & ty, other & ty & ~kn]
            got, want = out_new[i, side], out_old[i, side]
            for c in range(4):
                slack = int((near & cols[c]).sum())
                assert abs(int(got[c]) - int(want[c])) <= slack, (i, side, c, got, want, slack)
                flips += int(got[c] != want[c])
                elig = key_cols[c] & below
                if got[4 + c] != want[4 + c]:
                    m = sc[elig].min() if elig.any() else None
                    movable = (near & key_cols[c]).any() or got[c] != want[c] or \
                        (m is not None and (np.abs(sc[elig] - m) <= 64 * np.spacing(np.float32(m))).sum() > 1)
                    assert movable, (i, side, c, got, want)
    return flips


# ---------------------------------------------------------------------------------------------------------------------------
# 1-4: one process
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [12, 24, 48, 100, 200, 512, 520])
@pytest.mark.parametrize("test_head", [True, False])
def test_whole_table_as_one_range_matches_the_ranker(dim, test_head):
    require_entry_points()
    con = make_config(dim)
    E = con.entTotal
    new, _, _ = lp_ranges(con, [(0, E)], test_head=test_head)
    old, _ = con.link_prediction(0, None, test_head=test_head)
    if not test_head:
        assert not new[:, 1].any()
    flips = check_near_tie_rule(con, KG, new, old, test_head)
    assert flips <= 4


def cuts(E):
    return {
        1: [(0, E)],
        2: [(0, E // 2), (E // 2, E)],
        3: [(0, 333), (333, 334), (334, E)],
        7: [(0, 1), (1, 1), (1, 137), (137, 400), (400, 401), (401, 777), (777, E)],
    }


@pytest.mark.parametrize("dim", [48, 200])
def test_any_cut_of_the_table_gives_the_same_bits(dim):
    require_entry_points()
    con = make_config(dim)
    E = con.entTotal
    ref_out, ref_c, ref_k = lp_ranges(con, cuts(E)[1])
    assert ref_c.sum() > 0 and (ref_k != NO_KEY).any()
    for n, parts in cuts(E).items():
        out, c, k = lp_ranges(con, parts)
        assert np.array_equal(c, ref_c), n
        assert np.array_equal(k, ref_k), n
        assert np.array_equal(out, ref_out), n
    # a subrange of the test set and the tail side only: the same rows
    out, c, _ = lp_ranges(con, cuts(E)[7], first=5, count=11, test_head=False)
    assert np.array_equal(c[:, 0], ref_c[5:16, 0]) and not c[:, 1].any()
    assert np.array_equal(out[:, 0], ref_out[5:16, 0])


def test_a_copy_of_the_target_row_ties_and_is_never_counted():
    require_entry_points()
    con = make_config(48)
    E = con.entTotal
    hs, ts, _ = sorted_test_triples(KG)
    i = 0
    ent = con._tables[0]
    for side, target in ((0, int(ts[i])), (1, int(hs[i]))):
        # a stand-in in the other half of the table from the target, not an entity of triple i
        x = next(j for j in (range(E - 1, 0, -1) if target < E // 2 else range(1, E)) if j not in (int(hs[i]), int(ts[i])))
        base = {n: lp_ranges(con, parts)[1] for n, parts in cuts(E).items()}
        alone = lp_ranges(con, [(x, x + 1)])[1][i, side]      # what x itself adds with its own row
        saved = ent[x].clone()
        ent[x] = ent[target]           # the same bits as the target's row
        con.tables_changed()
        _, c, k = lp_ranges(con, [(x, x + 1)])
        assert not c[i, side].any() and (k[i, side] == NO_KEY).all(), side
        for n, parts in cuts(E).items():
            _, c, k = lp_ranges(con, parts)
            assert np.array_equal(c[i, side], base[n][i, side] - alone), (side, n)
            assert (key_ids(k[i, side]) != x).all(), (side, n)
        ent[x] = saved
        con.tables_changed()


@pytest.fixture(scope="module")
def typed_graph(tmp_path_factory):
    from openkeonspark_amd import synthetic
    return synthetic.make_typed_dataset(str(tmp_path_factory.mktemp("typed_lp")), synthetic.SMALL_TYPED)


@pytest.mark.parametrize("graph", ["kg_small", "typed"])
def test_filtered_typed_and_ontology_columns(graph, typed_graph):
    require_entry_points()
    path = KG if graph == "kg_small" else typed_graph
    con = make_config(32, path=path)
    E = con.entTotal
    old, _ = con.link_prediction(0, None, test_head=True)
    assert old[:, :, 1:4].sum() > 0
    outs = []
    for parts in ([(0, E)], [(0, E // 3), (E // 3, E // 3 + 1), (E // 3 + 1, E)], [(lo, min(lo + 97, E)) for lo in range(0, E, 97)]):
        out, _, _ = lp_ranges(con, parts)
        outs.append(out)
        assert np.array_equal(out, outs[0])
    check_near_tie_rule(con, path, outs[0], old, True)


# ---------------------------------------------------------------------------------------------------------------------------
# 5-7: ranks (gloo, one GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out_dir, data):
    import openkeonspark_amd as pkg
    con = start_rank(rank, world, port, data)
    total = con.lib.getTestTotal()
    res = {}
    res["dist"] = con.link_prediction_distributed()
    out_all, m_all = con.link_prediction()
    out_part, _ = con.link_prediction(3, 17)
    out_tail, m_tail = con.link_prediction(0, total, test_head=False)
    con.lp_shard_query_bytes = 5 * 2 * 48 * 4          # five triples per chunk
    out_chunked, _ = con.link_prediction()
    res["all"], res["tail"] = m_all, m_tail
    # test_step: every rank its own ids -- ids of every owner, repeats -- and the last rank none
    E, chunk = con.entTotal, con._shard["chunk"]
    rng = np.random.default_rng(100 + rank)
    if rank == world - 1:
        h = t = r = np.zeros(0, dtype=np.int64)
    else:
        n = 40 + 7 * rank
        h = rng.integers(0, E, n); t = rng.integers(0, E, n); r = rng.integers(0, con.relTotal, n)
        h[:world] = [min(g * chunk, E - 1) for g in range(world)]
        t[:world] = [min((g + 1) * chunk - 1, E - 1) for g in range(world)]
        h[world:2 * world] = h[:world]; t[world:2 * world] = h[:world]       # repeated ids
    scores = con.test_step(h, t, r)
    refused = 0
    for fn in (con.predict_tail_entity, con.predict_head_entity):
        try:
            fn(0, 0, 5)
        except pkg.KgeError as e:
            refused += "link_prediction" in str(e)
    finish_rank(con, out_dir, world, rank, out_all=out_all, out_part=out_part, out_tail=out_tail, out_chunked=out_chunked,
                h=h, t=t, r=r, scores=scores, refused=refused, metrics=json.dumps(res))


@pytest.fixture(scope="module")
def sharded_runs(tmp_path_factory):
    require_entry_points()
    return run_worlds(_rank_worker, tmp_path_factory.mktemp("lp_shard_ranks"), 31900 + os.getpid() % 1000)


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_equal_one_process_over_the_union_table(sharded_runs, world):
    base, data = sharded_runs
    zs = load_ranks(base, world)
    con = union_config(data, zs[0])
    assert con.entTotal == 1003 and con.entTotal % world
    total = con.lib.getTestTotal()
    want, _, _ = lp_ranges(con, [(0, con.entTotal)])
    want_tail, _, _ = lp_ranges(con, [(0, con.entTotal)], test_head=False)
    ref_keys = set(con.link_prediction()[1])          # the non-sharded method's metric names
    assert len(ref_keys) == 40
    for g, z in enumerate(zs):
        assert np.array_equal(z["ent"], zs[0]["ent"]) and np.array_equal(z["rel"], zs[0]["rel"])
        assert np.array_equal(z["out_all"], want), g
        assert np.array_equal(z["out_chunked"], want), g
        assert np.array_equal(z["out_part"], want[3:20]), g
        assert np.array_equal(z["out_tail"], want_tail), g
        m = json.loads(str(z["metrics"]))
        assert m == json.loads(str(zs[0]["metrics"]))
        assert set(m["dist"]) == ref_keys and set(m["all"]) == ref_keys
        assert m["dist"] == m["all"]
        sums = rank_eval.normalise(rank_eval.lp_sums(want, True), total)
        assert m["all"] == pytest.approx(sums, rel=0, abs=0)


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_test_step_scores_bit_for_bit(sharded_runs, world):
    base, data = sharded_runs
    zs = load_ranks(base, world)
    con = union_config(data, zs[0])
    for g, z in enumerate(zs):
        if len(z["h"]) == 0:           # (the rank that passed no triples took part in the exchange and got no scores)
            assert z["scores"].shape == (0,)
            continue
        want = con.test_step(z["h"], z["t"], z["r"])
        assert z["scores"].shape == want.shape == (len(z["h"]),)
        assert np.array_equal(z["scores"].view(np.uint32), want.view(np.uint32)), g
    assert len(zs[-1]["h"]) == 0 and len(zs[0]["h"]) > 0


@pytest.mark.parametrize("world", [2, 4])
def test_predict_entity_helpers_refuse_a_sharded_table(sharded_runs, world):
    base, _ = sharded_runs
    for z in load_ranks(base, world):
        assert int(z["refused"]) == 2


# ---------------------------------------------------------------------------------------------------------------------------
# 8: the driver
# ---------------------------------------------------------------------------------------------------------------------------
def _driver_worker(rank, world, port, out_dir, mode, run):
    sys.path.insert(0, ROOT)
    env = {"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world),
           "LOCAL_RANK": str(rank), "KGE_SINGLE_DEVICE": "1", "KGE_DIST_BACKEND": "gloo", "KGE_COUNTS_MIN_RECORDS": "0"}
    os.environ.update(env)
    from openkeonspark_amd import _lib
    from openkeonspark_amd import distribute_training as dt
    _lib.lib().kge_set_option(b"inv_table_max_bytes", 0)
    args = ["--input_path", KG, "--output_path", os.path.join(out_dir, run), "--embedding_dimension", "32",
            "--n_mini_batches", "5", "--ent_neg_rate", "3", "--alpha", "0.05", "--optimizer", "SGD", "--bern_flag", "1",
            "--train_times", "4", "--sparse_rows", "1", "--mode", mode, "--test_head", "1"]
    dt.main_fun(dt.parse_args(args))


def test_driver_mode_test_on_a_sharded_checkpoint(tmp_path):
    require_entry_points()
    import shutil
    import torch.multiprocessing as mp
    port = 32900 + os.getpid() % 1000
    mp.start_processes(_driver_worker, args=(2, port, str(tmp_path), "train", "model"), nprocs=2, join=True, start_method="spawn")
    assert any(".shard" in f for f in os.listdir(str(tmp_path / "model")))
    results = {}
    for i, w in enumerate((2, 4, 1)):
        run = "test%d" % w
        shutil.copytree(str(tmp_path / "model"), str(tmp_path / run))
        if w > 1:
            mp.start_processes(_driver_worker, args=(w, port + 1 + i, str(tmp_path), "test", run), nprocs=w, join=True,
                               start_method="spawn")
        else:
            mp.start_processes(_driver_worker, args=(1, port + 1 + i, str(tmp_path), "test", run), nprocs=1, join=True,
                               start_method="spawn")
        with open(str(tmp_path / run / "lp_results.json"), "rb") as f:
            results[w] = f.read()
    assert results[2] == results[4]
    sharded, single = json.loads(results[2]), json.loads(results[1])
    assert set(sharded) == set(single) and len(single) == 40
    n = 40   # test triples of kg_small: a near-tie flips one count of one triple, moving a metric by at most 1 / n
    for k in single:
        assert abs(sharded[k] - single[k]) <= 2.0 / n + 1e-12, (k, sharded[k], single[k])
