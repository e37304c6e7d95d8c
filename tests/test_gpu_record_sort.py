"""The two-launch record sort (csrc/transe_counts.hip bkt_tile_kernel + bkt_merge_kernel, engine option counts_sort_tiles = 1, the
default) against numpy and against the three-launch form it replaces (counts_sort_tiles = 0) on the same keys, through the test
hook kge_counts_sort_test; then whole training steps under both option values.

Everything the sort promises is exact, so every check of it is: the sorted keys, that every id carries its key, that the ids are a
permutation of the live indices, the bucket starts, the row span of EVERY key of the row space (empty ones included) and the
multiset of pieces.  The order of the ids inside a key is unspecified in both forms and nothing here looks at it.

T = 2048 keys is the tile of the first launch, 512 the number of buckets, 256 * 8 the pairs of a bucket that the second launch
holds in registers.  The shapes are the smallest at which each mechanism can break; each is listed with its reason at CASES."""
import ctypes

import numpy as np
import pytest

from test_gpu_models import RTOL, batch_without_ties, make_engine, rand_batch, relerr, seed_of

pytestmark = pytest.mark.gpu

T, NB = 2048, 512
CAP = 4          # plan capacity: lists of more than four records are cut into pieces


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    L.kge_set_option(b"counts_sort_tiles", 1)


def run_sort(L, tiles, keys, rows, rpb, cap):
    L.kge_set_option(b"counts_sort_tiles", tiles)
    M = len(keys)
    out = dict(keys=np.full(M, -9, np.int32), ids=np.full(M, -9, np.int32), n_live=np.full(1, -9, np.int32),
               bucket_start=np.full(NB + 2, -9, np.int32), row_span=np.full((rows, 2), -9, np.int32),
               pieces=np.full((M + 16, 4), -9, np.int32), n_pieces=np.full(1, -9, np.int32))
    rc = L.kge_counts_sort_test(keys.ctypes.data, M, rows, rpb, cap, out["keys"].ctypes.data, out["ids"].ctypes.data,
                                out["n_live"].ctypes.data, out["bucket_start"].ctypes.data, out["row_span"].ctypes.data,
                                out["pieces"].ctypes.data, M + 16, out["n_pieces"].ctypes.data, None)
    assert rc == 0, rc
    return out


def check_sorted(keys, rows, rpb, cap, got):
    live = np.nonzero(keys >= 0)[0]
    n = len(live)
    want = np.sort(keys[live])
    assert int(got["n_live"][0]) == n
    assert np.array_equal(got["keys"][:n], want)
    ids = got["ids"][:n]
    assert np.array_equal(np.sort(ids), live)                       # a permutation of the live indices ...
    assert np.array_equal(keys[ids], got["keys"][:n])               # ... each with its own key
    starts = np.searchsorted(want, np.arange(NB + 1, dtype=np.int64) * rpb, side="left")
    assert np.array_equal(got["bucket_start"][:NB + 1], starts)
    assert int(got["bucket_start"][NB]) == n
    if not cap:
        return
    first = np.searchsorted(want, np.arange(rows), side="left")
    count = np.searchsorted(want, np.arange(rows), side="right") - first
    assert np.array_equal(got["row_span"][:, 1], count)
    assert np.array_equal(got["row_span"][:, 0], first)             # empty keys included: where their records would lie
    # pieces from the definition: a key with records whose own list or whose row's other list (key ^ 1) is longer than cap
    other = np.zeros(rows, np.int64)
    k = np.arange(rows)
    inside = (k ^ 1) < rows
    other[inside] = count[(k ^ 1)[inside]]
    want_pieces = []
    for key in np.nonzero((count > 0) & ((count > cap) | (other > cap)))[0].tolist():
        c = int(count[key])
        want_pieces += [(key, int(first[key]) + q, min(cap, c - q), 0) for q in range(0, c, cap)]
    np_ = int(got["n_pieces"][0])
    assert np_ == len(want_pieces)
    assert sorted(map(tuple, got["pieces"][:np_].tolist())) == sorted(want_pieces)


def hub_keys(rng, M, rows, dead=0.6):
    """Zipf-like keys over the row space (hubs: lists longer than CAP), a fraction `dead` of them -1."""
    k = (rows * rng.random(M) ** 3).astype(np.int32)
    k[rng.random(M) < dead] = -1
    return k


def relation_pattern(rng):
    """The fused step's slot-major layout at 28 slots of 2 400 groups: slot 2 holds only relation keys, confined to the 31 buckets
    below the last one; slots 0 and 1 hold entity keys, the 25 negative slots entity keys of the other kind, two thirds dead."""
    Bq, rows, rpb = 2400, 30978, 62
    ent_keys = 29000
    slots = [2 * rng.integers(0, ent_keys // 2, Bq) for _ in range(2)]
    slots.append(rng.integers(rows - 32 * rpb, rows - rpb, Bq))
    for _ in range(25):
        s = 2 * rng.integers(0, ent_keys // 2, Bq) + 1
        s[rng.random(Bq) < 2 / 3] = -1
        slots.append(s)
    return np.concatenate(slots).astype(np.int32), rows, rpb


def make_case(name):
    rng = np.random.default_rng(seed_of("record-sort", name))
    if name.startswith("M="):                                   # one key, a tile less one, a full tile, one over, several and a ragged one
        M = {"M=1": 1, "M=T-1": T - 1, "M=T": T, "M=T+1": T + 1, "M=3T+7": 3 * T + 7}[name]
        return hub_keys(rng, M, 1000, 0.6 if M > 1 else 0.0), 1000, 2
    if name == "all-dead":
        return np.full(3 * T + 7, -1, np.int32), 1000, 2
    if name == "all-equal":                                     # one bucket takes whole tiles: 6 151 pairs > 256 * 8 in registers
        return np.full(3 * T + 7, 5, np.int32), 1000, 2
    if name == "last-row":                                      # rows % rpb != 0, the buckets behind the 251st empty
        return np.full(T + 1, 1000, np.int32), 1001, 4
    if name == "two-rows":
        return rng.integers(-1, 2, T + 1).astype(np.int32), 2, 2
    if name == "many-tiles":                                    # more tiles than threads in a workgroup of the bucket pass
        return hub_keys(rng, 257 * T + 5, 30978, 2 / 3), 30978, 62
    assert name == "relation-pattern"
    return relation_pattern(rng)


CASES = ["M=1", "M=T-1", "M=T", "M=T+1", "M=3T+7", "all-dead", "all-equal", "last-row", "two-rows", "many-tiles", "relation-pattern"]


@pytest.mark.parametrize("name", CASES)
def test_sort_against_numpy_and_the_three_launch_form(lib, name):
    keys, rows, rpb = make_case(name)
    assert rows <= NB * rpb
    plain = run_sort(lib, 1, keys, rows, rpb, 0)
    check_sorted(keys, rows, rpb, 0, plain)
    new = run_sort(lib, 1, keys, rows, rpb, CAP)
    check_sorted(keys, rows, rpb, CAP, new)
    old = run_sort(lib, 0, keys, rows, rpb, CAP)
    check_sorted(keys, rows, rpb, CAP, old)
    n, np_ = int(new["n_live"][0]), int(new["n_pieces"][0])
    assert np.array_equal(old["keys"][:n], new["keys"][:n])
    assert np.array_equal(old["bucket_start"][:NB + 1], new["bucket_start"][:NB + 1])
    assert np.array_equal(old["row_span"][:, 1], new["row_span"][:, 1])
    assert sorted(map(tuple, old["pieces"][:np_].tolist())) == sorted(map(tuple, new["pieces"][:np_].tolist()))
    if name in ("all-equal", "many-tiles", "relation-pattern", "M=3T+7"):
        assert np_ > 0                                          # pieces do appear


# ---- whole steps ----
E, R, TRAIN, W = 500, 7, 2400, 8          # one batch of 2 400 groups: 2 400 * 28 = 67 200 >= 65 536 records, the sign-count path
SEEDS = np.array([1804289383, 846930886, 1681692777, 1714636915, 1957747793, 424238335, 719885386, 1649760492], np.uint64)


@pytest.fixture(scope="module")
def kg_dir(tmp_path_factory):
    from openkeonspark_amd.synthetic import write_openke_dir
    rng = np.random.default_rng(8)
    seen = set()
    while len(seen) < TRAIN:
        seen.add((int(rng.integers(0, E)), int(rng.integers(0, E)), int(rng.integers(0, R))))
    tri = np.array(sorted(seen), np.int64)
    tri = tri[rng.permutation(len(tri))]
    path = str(tmp_path_factory.mktemp("record_sort_kg")) + "/"
    write_openke_dir(path, E, R, tri[:, 0], tri[:, 1], tri[:, 2])
    return path


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def run_steps(L, tiles, path, D, opt, params):
    import torch
    from openkeonspark_amd.Config import Config
    import openkeonspark_amd as pkg
    L.kge_set_option(b"counts_sort_tiles", tiles)
    con = Config()
    con.prefetch_sampling = True            # the next batch's sampler rides in the sort's first launch
    con.set_in_path(path); con.set_work_threads(W); con.set_bern(1)
    con.set_dimension(D); con.set_nbatches(1)
    con.set_ent_neg_rate(25); con.set_rel_neg_rate(0); con.set_margin(0.5)
    con.set_opt_method(opt); con.set_alpha(0.001 if opt == "Adam" else 0.01)
    con.init()
    con.set_model_and_session(pkg.TransE)
    assert con.batch_size == TRAIN and con.batch_size * 28 >= 65536 and con.use_counts and not con.sparse_rows
    con.set_parameters(params)
    assert con.lib.kge_set_stream_states(SEEDS.ctypes.data, W) == 0
    losses = [np.float32(con.train_step()).tobytes() for _ in range(3)]
    torch.cuda.synchronize()
    out = {k: v.copy() for k, v in con.get_parameters().items()}
    if opt == "Adam":
        for i, k in enumerate(con.trainModel.table_names):
            out["m/" + k] = con._adam_m[i].cpu().numpy()
            out["v/" + k] = con._adam_v[i].cpu().numpy()
    return losses, out


@pytest.mark.parametrize("D,opt", [(200, "Adam"), (100, "SGD")])
def test_training_steps_equal_bit_for_bit(lib, kg_dir, D, opt):
    """Three steps from the same tables and sampler state: loss, both tables and both moments, under counts_sort_tiles 0 and 1."""
    rng = np.random.default_rng(D)
    params = {"ent_embeddings": rng.standard_normal((E, D)).astype(np.float32),
              "rel_embeddings": rng.standard_normal((R, D)).astype(np.float32)}
    old_losses, old = run_steps(lib, 0, kg_dir, D, opt, params)
    new_losses, new = run_steps(lib, 1, kg_dir, D, opt, params)
    assert old_losses == new_losses
    assert set(old) == set(new) and len(old) == (6 if opt == "Adam" else 2)
    for k in old:
        assert np.array_equal(bits(old[k]), bits(new[k])), k
    assert not np.array_equal(new["ent_embeddings"], params["ent_embeddings"])


def test_transh_pair_count_step_under_both_forms(lib):
    """One TransH step on the pair-count path (its keys go through the same sort; its float sums may differ in order, as they can
    between two runs): against the oracle to the tolerance tests/test_gpu_models.py::test_pair_count_path_shapes uses."""
    import torch
    from oracle import oracle
    model, E_, R_, D, B, n = "transh", 300, 7, 132, 257, 16
    rng = np.random.default_rng(seed_of(model, E_, R_, D, B, n, "record-sort"))
    params = oracle.init_params(oracle.MODEL_IDS[model], E_, R_, D, D, seed=14)
    for k in params:
        params[k] = (params[k] * 3).astype(np.float32)
    orc = oracle.Model(model, E_, R_, D, D, margin=1.0, params=params)
    bh, bt, br = batch_without_ties(orc, lambda: rand_batch(rng, E_, R_, B, n, 0, 0.05), B, n)
    loss_o, g_o = orc.grad(bh, bt, br, B, n)
    lib.kge_set_option(b"float_records_min", 0)
    lib.kge_set_option(b"pair_counts_min_neg", 1)
    try:
        for tiles in (0, 1):
            lib.kge_set_option(b"counts_sort_tiles", tiles)
            con = make_engine(model, E_, R_, D, n, 0, params=params)
            dev = torch.from_numpy(np.stack([bh, bt, br]).astype(np.int32)).cuda()
            con.forward_backward(dev, B, B, B * n)
            torch.cuda.synchronize()
            assert abs(float(con._loss.item()) - loss_o) <= RTOL * abs(loss_o), tiles
            g_g = con.get_gradients()
            for k in g_o:
                assert relerr(g_g[k], g_o[k]) < RTOL, (tiles, k, relerr(g_g[k], g_o[k]))
    finally:
        lib.kge_set_option(b"float_records_min", 1 << 16)
        lib.kge_set_option(b"pair_counts_min_neg", 0)
