"""The sampler's table jumps, table moduli, single pick path and wide filter-list search (csrc/sampler_dev.hpp lcg_skip_tab,
filtered_pick_wide) against the pinned oracle: h, t, r and the stream states bit for bit over three consecutive calls.

Graph (b): 1000 entities, 4 relations.  Heads 0..9 have, under relation 0, known-tail groups of 4, 5, 8, 9, 24, 25, 80, 81, 600
and 999 (= E - 1) ids, and tails 10..19 the same known-head groups under relation 1: for a fan of m = 4 or m = 8 pivots per level
these are m, m + 1, (m + 1)^2 - 1 and (m + 1)^2 -- the lengths at which the search gains a level -- besides the short lists, a
long one and the group that leaves one candidate.  A positive is picked uniformly among the triples, so the long groups are the
ones searched most.  No (h, t) pair carries all four relations (the reference divides by zero there)."""
import ctypes

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import oracle

pytestmark = pytest.mark.gpu

E, R = 1000, 4
LENGTHS = [4, 5, 8, 9, 24, 25, 80, 81, 600, E - 1]
CALLS = 3


def build_graph():
    rng = np.random.default_rng(7)
    tri = set()
    for i, n in enumerate(LENGTHS):
        for x in rng.choice(E, n, replace=False):
            tri.add((i, int(x), 0))                 # tails(i, r0) has n ids
        for x in rng.choice(E, n, replace=False):
            tri.add((int(x), 10 + i, 1))            # heads(10 + i, r1) has n ids
    for _ in range(400):                            # background of short groups; relation 3 stays rare
        tri.add((int(rng.integers(20, E)), int(rng.integers(20, E)), 2 + int(rng.integers(0, 8) == 0)))
    tri = np.array(sorted(tri), np.int64)
    tri = tri[rng.permutation(len(tri))]
    rels = {}
    for h, t, r in tri:
        rels.setdefault((h, t), set()).add(r)
    assert max(len(v) for v in rels.values()) < R
    return tri


@pytest.fixture(scope="module")
def graph_dir(tmp_path_factory):
    from openkeonspark_amd.synthetic import write_openke_dir
    tri = build_graph()
    path = str(tmp_path_factory.mktemp("sampler_tables_kg")) + "/"
    write_openke_dir(path, E, R, tri[:, 0], tri[:, 1], tri[:, 2])
    return path


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    L.kge_set_option(b"sampler_magic_len", 2048)
    L.kge_set_option(b"ride_shares", 100 << 8)


def make_config(path, W, bern):
    from openkeonspark_amd.Config import Config
    con = Config()
    con.set_in_path(path)
    con.set_work_threads(W)
    con.set_bern(bern)
    con.init()
    return con


def abi_sampling(con, B, n, nr):
    from openkeonspark_amd import _lib
    tot = B * (1 + n + nr)
    h = np.zeros(tot, np.int64); t = np.zeros(tot, np.int64); r = np.zeros(tot, np.int64)
    y = np.zeros(tot, np.float32)
    con.lib.kge_clear_error()
    con.lib.sampling(h.ctypes.data, t.ctypes.data, r.ctypes.data, y.ctypes.data, B, n, nr)
    _lib.raise_if_error(con.lib)
    return h, t, r


def check_against_oracle(path, W, bern, B, n, nr, what=()):
    kg = oracle.KG(path, work_threads=W, bern=bern)
    con = make_config(path, W, bern)
    seeds = np.ascontiguousarray(kg.stream_states())
    assert con.lib.kge_set_stream_states(seeds.ctypes.data, W) == 0
    for c in range(CALLS):
        want = kg.sampling(B, n, nr)
        got = abi_sampling(con, B, n, nr)
        for name, a, b in zip("htr", got, want):
            assert np.array_equal(a, b), what + (W, bern, B, n, nr, c, name)
    assert con.get_stream_states().tolist() == kg.stream_states().tolist(), what + (W, B, n, nr)
    return con


def test_group_lengths_of_the_generated_graph(graph_dir):
    """the graph holds what its description says (host index only)"""
    con = make_config(graph_dir, 1, 0)
    nbytes = con.lib.kge_index_copy(b"grp", None, 0)
    grp = np.zeros(nbytes // 4, np.int32)
    con.lib.kge_index_copy(b"grp", grp.ctypes.data, nbytes)
    grp = grp.reshape(-1, 4)
    for n in LENGTHS:
        assert (grp[:, 1] >= n).any() and (grp[:, 3] >= n).any()
    assert set(LENGTHS[:4]) <= set(grp[:, 1].tolist()) and grp[:, 1].max() == E - 1 and grp[:, 3].max() == E - 1


@pytest.mark.parametrize("kg_name", ["kg_tiny", "kg_small", "kg_incr"])
def test_golden_graphs(lib, kg_name):
    import os
    for W, bern, B, n, nr in [(3, 0, 50, 3, 0), (8, 1, 64, 25, 0), (8, 1, 64, 2, 1)]:
        check_against_oracle(os.path.join(GOLDEN, kg_name), W, bern, B, n, nr)


@pytest.mark.parametrize("magic_len", [8, 2048])
def test_long_groups_with_table_and_fallback_moduli(lib, graph_dir, magic_len):
    """magic_len = 8: groups of 4 and 5 ids take their modulus from the table and every longer one the fp64 fallback;
    2048 (the default): all of them the table, the E - 1 group with divisor 1 included."""
    assert lib.kge_set_option(b"sampler_magic_len", magic_len) == 0
    for W, bern, B, n, nr in [(8, 1, 300, 25, 0), (2, 0, 257, 3, 2)]:
        check_against_oracle(graph_dir, W, bern, B, n, nr, (magic_len,))


JUMP_CASES = [(1, 600, 1, 0),        # 3 draws per positive: the slice offset crosses the first digit (512)
              (1, 2100, 63, 0),      # 127 draws per positive: 266 700 draws, past 2^18 -- the third digit
              (1, 2100, 63, 63),     # 127 slots per positive: the one-thread-per-slot sampler, per-lane jumps
              (3, 100, 1, 0)]        # slices of 34: B % W != 0, and a wave (32 positives) reaches into the next slice


@pytest.mark.parametrize("W,B,n,nr", JUMP_CASES)
def test_jump_ranges(lib, graph_dir, W, B, n, nr):
    check_against_oracle(graph_dir, W, 1, B, n, nr)


def test_thread_range_that_starts_inside_the_batch(lib, graph_dir):
    """kge_sampling_device for virtual threads [3, 8) of 8: the launch's first position is 3 slices into the batch"""
    import torch
    W, B, n, nr = 8, 1001, 25, 0
    kg = oracle.KG(graph_dir, work_threads=W, bern=1)
    con = make_config(graph_dir, W, 1)
    seeds = np.ascontiguousarray(kg.stream_states())
    assert con.lib.kge_set_stream_states(seeds.ctypes.data, W) == 0
    for c in range(CALLS):
        rh, rt, rr, _ = kg.sampling(B, n, nr)
        first, nl = ctypes.c_int64(), ctypes.c_int64()
        cnt = int(con.lib.kge_slice_positions(B, 3, W, ctypes.byref(first)))
        assert first.value == 3 * 126 and cnt == B - first.value
        buf = torch.zeros((3, cnt * (1 + n)), dtype=torch.int32, device="cuda")
        assert con.lib.kge_sampling_device(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), B, n, nr, 3, W, cnt,
                                           ctypes.byref(nl), None) == 0 and nl.value == cnt
        host = buf.cpu().numpy().reshape(3, 1 + n, cnt)
        for a, want in zip(host, (rh, rt, rr)):
            assert np.array_equal(a, want.reshape(1 + n, B)[:, first.value:]), c
        assert con.get_stream_states().tolist() == kg.stream_states().tolist()


def prefetch_step(L, path, shares):
    """One TransE step whose scatter launch carries the next batch's sampler (shares = the default) or leaves it to a launch of
    its own (0) -> the batch drawn ahead, its pack, the stream states."""
    import torch
    import openkeonspark_amd as pkg
    from openkeonspark_amd.Config import Config
    L.kge_set_option(b"ride_shares", shares)
    con = Config()
    con.counts_min_records = 0          # this small step takes the sign-count path, whose launches carry the sampler
    con.prefetch_sampling = True
    con.set_in_path(path); con.set_work_threads(8); con.set_bern(1)
    con.set_dimension(200); con.set_nbatches(8)
    con.set_ent_neg_rate(25); con.set_margin(0.5)
    con.set_opt_method("Adam"); con.set_alpha(0.001)
    con.init()
    con.set_model_and_session(pkg.TransE)
    assert con.use_counts
    rng = np.random.default_rng(3)
    con.set_parameters({"ent_embeddings": rng.standard_normal((E, 200)).astype(np.float32),
                        "rel_embeddings": rng.standard_normal((R, 200)).astype(np.float32)})
    kg = oracle.KG(path, work_threads=8, bern=1)
    seeds = np.ascontiguousarray(kg.stream_states())
    assert con.lib.kge_set_stream_states(seeds.ctypes.data, 8) == 0
    loss = np.float32(con.train_step()).tobytes()
    torch.cuda.synchronize()
    buf, n_pos, _ = con._prefetched
    assert con._dev_pack is not None
    return dict(loss=loss, batch=buf.cpu().numpy(), n_pos=n_pos, pack=con._dev_pack[con._slot].cpu().numpy(),
                states=con.get_stream_states().tolist(), B=con.batch_size, kg=kg)


def test_riding_sampler_draws_the_batch_of_its_own_launch(lib, graph_dir):
    ride = prefetch_step(lib, graph_dir, 100 << 8)
    own = prefetch_step(lib, graph_dir, 0)
    assert ride["n_pos"] == own["n_pos"] == ride["B"]
    assert ride["loss"] == own["loss"]
    assert np.array_equal(ride["batch"], own["batch"]) and np.array_equal(ride["pack"], own["pack"])
    assert ride["states"] == own["states"]
    # and it is the oracle's second batch
    kg, B = ride["kg"], ride["B"]
    kg.sampling(B, 25, 0)
    want = kg.sampling(B, 25, 0)
    for a, b in zip(ride["batch"], want):
        assert np.array_equal(a[:B * 26], b)
    assert ride["states"] == kg.stream_states().tolist()
