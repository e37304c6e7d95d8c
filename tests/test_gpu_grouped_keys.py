"""Group-major record keys in the fused single-process TransE step (engine option emit_keys_grouped = 1, the default: the round body
of csrc/models.hip writes a group's S = 3 + n_neg keys side by side, dst[b * S + slot], and the tile pass of the two-launch record
sort -- csrc/transe_counts.hip bkt_tile_kernel<T, true> -- turns a position p into the record id (p % S) * n_pos + p / S) against
the slot-major step it replaces (emit_keys_grouped = 0) on the same device-sampled batches.

Nothing but the place of a key in the engine's scratch changes, so everything is compared BIT FOR BIT: the loss of every step,
both tables, both Adam moments, the emit kernel's 1/|row| table and the keys as kge_transe_step_scratch_read hands them back
(slot-major under both values).

Shapes: S = 4, 28 and 66 (66 > 64 lanes: the group's keys need a second store); one group, and group counts that are no multiple
of the four teams of a workgroup; M = S * n_pos on either side of the sort's 2 048-key tile (73 / 74 groups of 28, 511 / 513 groups
of 4); widths 132, 200 and 256 (the round body) and 100 (another body, which keeps slot-major keys: the option must change
nothing).  Every shape runs with emit_pack, emit_rounds and counts_sort_tiles at 0 and at 1: without the pack the round body reads
the strided id arrays (another kernel), without emit_rounds or with the three-launch sort the step keeps slot-major keys."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, R, W = 100, 7, 8
NBATCH = 3
MARGIN = 0.5              # random rows: p - score spreads about +-1 around 0, so hinges fall on either side
SEEDS = np.array([1804289383, 846930886, 1681692777, 1714636915, 1957747793, 424238335, 719885386, 1649760492], np.uint64)
OPTIONS = (b"emit_keys_grouped", b"emit_pack", b"emit_rounds", b"counts_sort_tiles")


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    for name in OPTIONS:
        L.kge_set_option(name, 1)
    L.kge_set_option(b"counts_sort_test_group", 0)


def graph(n_pos, rels=R):
    """NBATCH * n_pos distinct triples over E entities and `rels` relations: NBATCH batches of n_pos groups."""
    rng = np.random.default_rng(1000 * n_pos + rels)
    seen = set()
    while len(seen) < NBATCH * n_pos:
        seen.add((int(rng.integers(0, E)), int(rng.integers(0, E)), int(rng.integers(0, rels))))
    tri = np.array(sorted(seen), np.int64)
    tri = tri[rng.permutation(len(tri))]
    return E, rels, tri[:, 0], tri[:, 1], tri[:, 2]


def tables(D, seed, rels=R):
    rng = np.random.default_rng(seed)
    return {"ent_embeddings": rng.standard_normal((E, D)).astype(np.float32),
            "rel_embeddings": rng.standard_normal((rels, D)).astype(np.float32)}


def make_config(arrays, n_pos, D, n, params):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.counts_min_records = 0          # these small steps take the sign-count path ...
    con.fused_counts = True             # ... and its fused form
    con.prefetch_sampling = True        # the next batch's sampler rides in the sort's launches
    con.set_work_threads(W); con.set_bern(1)
    con.set_dimension(D); con.set_nbatches(NBATCH)
    con.set_ent_neg_rate(n); con.set_rel_neg_rate(0); con.set_margin(MARGIN)
    con.set_opt_method("Adam"); con.set_alpha(0.001)
    con.init_from_arrays(*arrays)
    con.set_model_and_session(pkg.TransE)
    assert con.batch_size == n_pos and con.use_counts and not con.sparse_rows
    con.set_parameters(params)
    assert con.lib.kge_set_stream_states(SEEDS.ctypes.data, W) == 0
    return con


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def snapshot(L, con, n_pos, n):
    """Tables, moments, the 1/|row| table and the last step's keys."""
    import torch
    torch.cuda.synchronize()
    out = {k: v.copy() for k, v in con.get_parameters().items()}
    for i, k in enumerate(con.trainModel.table_names):
        out["m/" + k] = con._adam_m[i].cpu().numpy()
        out["v/" + k] = con._adam_v[i].cpu().numpy()
    keys = np.zeros(n_pos * (3 + n), np.int32)
    assert L.kge_transe_step_scratch_read(1, 0, keys.size, keys.ctypes.data) == 0
    out["keys"] = keys
    inv = np.zeros(con.entTotal + con.relTotal, np.float32)
    assert L.kge_transe_step_scratch_read(2, 0, inv.size, inv.ctypes.data) == 0
    out["1/|row|"] = inv
    return out


def run_steps(L, grouped, other, arrays, n_pos, D, n, params, steps=3):
    for name, v in zip(OPTIONS, (grouped,) + other):
        L.kge_set_option(name, v)
    con = make_config(arrays, n_pos, D, n, params)
    losses = [np.float32(con.train_step()).tobytes() for _ in range(steps)]
    return losses, snapshot(L, con, n_pos, n)


def compare(old, new, what):
    assert old[0] == new[0], what
    assert set(old[1]) == set(new[1]) and len(old[1]) == 8
    for k in old[1]:
        assert np.array_equal(bits(old[1][k]), bits(new[1][k])), (k,) + tuple(what)


# (n_neg, n_pos, D)
CASES = [(1, 1, 200), (1, 3, 132), (1, 5, 256), (1, 511, 200), (1, 513, 200),
         (25, 1, 132), (25, 3, 200), (25, 5, 256), (25, 73, 200), (25, 74, 200), (25, 74, 132), (25, 73, 256),
         (63, 1, 256), (63, 3, 200), (63, 5, 132),
         (25, 74, 100), (1, 513, 100)]
# emit_pack, emit_rounds, counts_sort_tiles: all on, and each of them off
VARIANTS = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)]


@pytest.mark.parametrize("n,n_pos,D", CASES)
def test_steps_equal_bit_for_bit(lib, n, n_pos, D):
    arrays = graph(n_pos)
    params = tables(D, 100 * D + n)
    for other in VARIANTS:
        what = (n, n_pos, D) + other
        old = run_steps(lib, 0, other, arrays, n_pos, D, n, params)
        new = run_steps(lib, 1, other, arrays, n_pos, D, n, params)
        compare(old, new, what)
        assert not np.array_equal(new[1]["ent_embeddings"], params["ent_embeddings"]), what
        if n_pos >= 73:
            neg = new[1]["keys"][3 * n_pos:]
            assert (neg >= 0).any() and (neg < 0).any(), what           # active and idle hinges


def test_one_relation(lib):
    """A graph with one relation: every group's relation key falls on the few copies of one row (lists cut into pieces)."""
    n, n_pos, D = 25, 74, 200
    arrays = graph(n_pos, rels=1)
    params = tables(D, 77, rels=1)
    for other in ((1, 1, 1), (0, 1, 1)):
        old = run_steps(lib, 0, other, arrays, n_pos, D, n, params)
        new = run_steps(lib, 1, other, arrays, n_pos, D, n, params)
        compare(old, new, ("one relation",) + other)
        assert not np.array_equal(new[1]["rel_embeddings"], params["rel_embeddings"])


def test_hand_fed_batch_with_a_deferred_group(lib):
    """A fed batch, sampler-shaped but for ONE group whose second negative differs from its positive in two slots: the emit kernel
    defers that group (all S keys -1) and the exact fp32 pass differentiates it -- one group, handled by one team, so its adds into
    the residual tables come in program order and the step stays bit-exact between the two layouts."""
    n, n_pos, D, odd = 25, 74, 200, 41
    rng = np.random.default_rng(3)
    h = rng.integers(0, E, n_pos); t = rng.integers(0, E, n_pos); r = rng.integers(0, R, n_pos)
    H, T, Rr = [h], [t], [r]
    for k in range(n):
        which = rng.integers(0, 2, n_pos)
        nh = np.where(which == 0, (h + 1 + rng.integers(0, E - 1, n_pos)) % E, h)
        nt = np.where(which == 1, (t + 1 + rng.integers(0, E - 1, n_pos)) % E, t)
        if k == 1:
            nh[odd] = (h[odd] + 1) % E; nt[odd] = (t[odd] + 1) % E
        H.append(nh); T.append(nt); Rr.append(r)
    bh, bt, br = [np.concatenate(x).astype(np.int64) for x in (H, T, Rr)]
    arrays = graph(n_pos)
    params = tables(D, 5)
    got = []
    for grouped in (0, 1):
        for name, v in zip(OPTIONS, (grouped, 1, 1, 1)):
            lib.kge_set_option(name, v)
        con = make_config(arrays, n_pos, D, n, params)
        losses = [np.float32(con.train_step(bh, bt, br, None)).tobytes() for _ in range(2)]
        deferred = ctypes.c_int32(-1)
        assert lib.kge_transe_deferred_groups(ctypes.byref(deferred)) == 0 and deferred.value == 1
        got.append((losses, snapshot(lib, con, n_pos, n)))
    compare(got[0], got[1], ("hand-fed",))
    keys = got[1][1]["keys"].reshape(3 + n, n_pos)
    assert (keys[:, odd] == -1).all()
    others = np.delete(keys, odd, axis=1)
    assert (others[:3] >= 0).any() and (others[3:] >= 0).any()
    assert not np.array_equal(got[1][1]["ent_embeddings"], params["ent_embeddings"])


T_KEYS, NB = 2048, 512


@pytest.mark.parametrize("S", [4, 28, 66])
def test_position_to_id_at_the_largest_tile_input(lib, S):
    """The tile pass's position -> record id translation (a multiply-high by a host-made magic) at the largest input the two-launch
    form takes, 2 048 tiles of 2 048 keys: every live pair (id, key) must be ((p % S) * n_pos + p / S, keys[p]) of a position p."""
    n_pos = (T_KEYS * T_KEYS) // S
    M, rows, rpb = n_pos * S, 30978, 62
    rng = np.random.default_rng(S)
    keys = rng.integers(0, rows, M).astype(np.int32)
    keys[rng.random(M) < 2 / 3] = -1
    keys[[0, M - 1]] = [5, rows - 1]                      # the first and the last position are live
    lib.kge_set_option(b"counts_sort_tiles", 1)
    lib.kge_set_option(b"counts_sort_test_group", S)
    out_keys, out_ids = np.full(M, -9, np.int32), np.full(M, -9, np.int32)
    n_live, bucket_start = np.full(1, -9, np.int32), np.full(NB + 2, -9, np.int32)
    rc = lib.kge_counts_sort_test(keys.ctypes.data, M, rows, rpb, 0, out_keys.ctypes.data, out_ids.ctypes.data, n_live.ctypes.data,
                                  bucket_start.ctypes.data, None, None, 0, None, None)
    assert rc == 0, rc
    p = np.nonzero(keys >= 0)[0]
    n = len(p)
    assert int(n_live[0]) == n
    want_ids = (p % S) * n_pos + p // S
    key_of_id = np.full(M, -1, np.int32)
    key_of_id[want_ids] = keys[p]
    assert np.array_equal(out_keys[:n], np.sort(keys[p]))
    assert np.array_equal(np.sort(out_ids[:n]), np.sort(want_ids))          # the ids of the live positions, each once ...
    assert np.array_equal(key_of_id[out_ids[:n]], out_keys[:n])             # ... each with the key of its position
