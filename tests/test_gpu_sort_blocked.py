"""The two-launch record sort with packed, block-major tile offsets and the XCD-affine bucket order (csrc/transe_counts.hip
bkt_tile_kernel / bkt_merge_kernel with G > 0, engine option counts_sort_blocked = 1, the default) against numpy, next to the
layout it replaces (counts_sort_blocked = 0) and the three-launch form (counts_sort_tiles = 0), through the test hook
kge_counts_sort_test; then whole training steps under both values of the option.

What is checked is what tests/test_gpu_record_sort.py checks, with its own check_sorted: the sorted keys, the ids a permutation of
the live indices that each carry their key, bucket_start[0 .. NB], the row span of EVERY key and the multiset of pieces; all of it
exact.  The order of the ids inside a key is unspecified and nothing here looks at it.

T = 2048 keys per tile, NB = 512 buckets, G = 8 buckets per block of offsets; the bucket pass hands workgroup i the bucket
(i % 8) * 64 + i / 8, so an XCD run is 64 consecutive buckets.  A cell's word is start | len << 16 with both <= T.  The shapes are the
smallest at which each of these can break; each is listed with its reason at make_case."""
import numpy as np
import pytest

from test_gpu_models import seed_of
from test_gpu_record_sort import CAP, NB, T, check_sorted, hub_keys, kg_dir, run_steps, bits, E, R  # noqa: F401 (kg_dir: fixture)

pytestmark = pytest.mark.gpu

G = 8
RPB = 4                      # rows per bucket of the bucket-targeted cases: key k lies in bucket k // RPB
ROWS = NB * RPB
# (counts_sort_tiles, counts_sort_blocked)
FORMS = {"blocked": (1, 1), "unblocked": (1, 0), "three-launch": (0, 1)}


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    L.kge_set_option(b"counts_sort_tiles", 1)
    L.kge_set_option(b"counts_sort_blocked", 1)


def run_sort(L, tiles, blocked, keys, rows, rpb, cap):
    L.kge_set_option(b"counts_sort_tiles", tiles)
    L.kge_set_option(b"counts_sort_blocked", blocked)
    M = len(keys)
    out = dict(keys=np.full(M, -9, np.int32), ids=np.full(M, -9, np.int32), n_live=np.full(1, -9, np.int32),
               bucket_start=np.full(NB + 2, -9, np.int32), row_span=np.full((rows, 2), -9, np.int32),
               pieces=np.full((M + 16, 4), -9, np.int32), n_pieces=np.full(1, -9, np.int32))
    rc = L.kge_counts_sort_test(keys.ctypes.data, M, rows, rpb, cap, out["keys"].ctypes.data, out["ids"].ctypes.data,
                                out["n_live"].ctypes.data, out["bucket_start"].ctypes.data, out["row_span"].ctypes.data,
                                out["pieces"].ctypes.data, M + 16, out["n_pieces"].ctypes.data, None)
    assert rc == 0, rc
    return out


def in_buckets(rng, M, buckets, dead=0.0):
    """M keys spread over the rows of the given buckets, a fraction `dead` of them -1."""
    k = (rng.choice(np.asarray(buckets), M) * RPB + rng.integers(0, RPB, M)).astype(np.int32)
    k[rng.random(M) < dead] = -1
    return k


def make_case(name):
    rng = np.random.default_rng(seed_of("sort-blocked", name))
    if name == "one-tile":                                     # n_tiles = 1: every block of offsets is G words long
        return hub_keys(rng, T, ROWS, 0.5), ROWS, RPB
    if name == "T+1":                                          # n_tiles = 2, the second tile holds one key
        k = hub_keys(rng, T + 1, ROWS, 0.5)
        k[T] = 1234
        return k, ROWS, RPB
    if name == "257-tiles":                                    # a bucket-pass thread owns two tiles: its reads lie 4 G bytes apart
        return hub_keys(rng, 257 * T + 5, 30978, 2 / 3), 30978, 62
    if name == "tile-in-one-bucket":                           # len = T, the largest value of the 16-bit field; start = T behind it
        k = hub_keys(rng, 3 * T, ROWS, 0.5)
        k[T:2 * T] = 201 * RPB + rng.integers(0, RPB, T)
        return k, ROWS, RPB
    if name == "dead-tile":                                    # a tile that publishes 512 words of start = 0, len = 0
        k = hub_keys(rng, 3 * T, ROWS, 0.5)
        k[T:2 * T] = -1
        return k, ROWS, RPB
    if name == "all-dead":
        return np.full(2 * T + 7, -1, np.int32), ROWS, RPB
    if name == "block-seam":                                   # the last bucket of one block of offsets and the first of the next
        return in_buckets(rng, 2 * T + 7, [G - 1, G], 0.3), ROWS, RPB
    if name == "block-seams-4-8-16":                           # the same for every block size that is compiled
        return in_buckets(rng, 2 * T + 7, [3, 4, 7, 8, 15, 16], 0.3), ROWS, RPB
    if name == "first-and-last-bucket":                        # workgroup 0 and workgroup NB - 1 (which writes bucket_start[NB])
        return in_buckets(rng, 2 * T + 7, [0, NB - 1], 0.3), ROWS, RPB
    if name == "xcd-run-heads":                                # the first bucket of each run of 64: workgroups 0 .. 7
        return in_buckets(rng, 2 * T + 7, list(range(0, NB, NB // 8)), 0.3), ROWS, RPB
    if name == "xcd-run-tails":                                # the last bucket of each run: workgroups NB - 8 .. NB - 1
        return in_buckets(rng, 2 * T + 7, list(range(NB // 8 - 1, NB, NB // 8)), 0.3), ROWS, RPB
    if name == "rows-end-inside-a-bucket":                     # bucket 300 holds one row; the workgroups of the buckets behind it leave early
        rows = 300 * RPB + 1
        k = hub_keys(rng, 2 * T + 7, rows, 0.3)
        k[5] = rows - 1
        return k, rows, RPB
    if name == "last-bucket-empty":                            # bucket_start[NB] = bucket_start[NB - 1]: the tail write of an empty bucket
        return in_buckets(rng, 2 * T + 7, list(range(NB - 1)), 0.3), ROWS, RPB
    assert name == "random"
    return hub_keys(rng, 3 * T + 7, 30978, 2 / 3), 30978, 62


CASES = ["one-tile", "T+1", "257-tiles", "tile-in-one-bucket", "dead-tile", "all-dead", "block-seam", "block-seams-4-8-16",
         "first-and-last-bucket", "xcd-run-heads", "xcd-run-tails", "rows-end-inside-a-bucket", "last-bucket-empty", "random"]


@pytest.mark.parametrize("name", CASES)
def test_sort_against_numpy_in_every_form(lib, name):
    keys, rows, rpb = make_case(name)
    assert rows <= NB * rpb and rpb % 2 == 0
    got = {}
    for form, (tiles, blocked) in FORMS.items():
        got[form] = run_sort(lib, tiles, blocked, keys, rows, rpb, CAP)
        check_sorted(keys, rows, rpb, CAP, got[form])
    check_sorted(keys, rows, rpb, 0, run_sort(lib, 1, 1, keys, rows, rpb, 0))      # the bucket pass without the plan
    new, old = got["blocked"], got["unblocked"]
    n, np_ = int(new["n_live"][0]), int(new["n_pieces"][0])
    assert np.array_equal(old["keys"][:n], new["keys"][:n])
    assert np.array_equal(old["bucket_start"][:NB + 2], new["bucket_start"][:NB + 2])
    assert np.array_equal(old["row_span"], new["row_span"])
    assert sorted(map(tuple, old["pieces"][:np_].tolist())) == sorted(map(tuple, new["pieces"][:np_].tolist()))
    if name in ("257-tiles", "tile-in-one-bucket", "random"):
        assert np_ > 0                                          # pieces do appear


@pytest.mark.parametrize("tiles,blocked", [(1, 4), (1, 16), (1024, 1), (4096, 1)])
@pytest.mark.parametrize("name", ["block-seams-4-8-16", "tile-in-one-bucket", "random"])
def test_measurement_block_and_tile_sizes(lib, name, tiles, blocked):
    """The block sizes 4 and 16 and the tile sizes 1024 and 4096 are compiled for measurements: they sort as well."""
    keys, rows, rpb = make_case(name)
    check_sorted(keys, rows, rpb, CAP, run_sort(lib, tiles, blocked, keys, rows, rpb, CAP))


@pytest.mark.parametrize("D,opt", [(200, "Adam"), (100, "SGD")])
def test_training_steps_equal_bit_for_bit(lib, kg_dir, D, opt):
    """Three steps from the same tables and sampler state on the sign-count path with the two-launch sort (the shape of
    tests/test_gpu_record_sort.py: one batch of 2 400 groups, 67 200 records): loss, both tables and both moments, under
    counts_sort_blocked 0 and 1."""
    rng = np.random.default_rng(D)
    params = {"ent_embeddings": rng.standard_normal((E, D)).astype(np.float32),
              "rel_embeddings": rng.standard_normal((R, D)).astype(np.float32)}
    lib.kge_set_option(b"counts_sort_blocked", 0)
    old_losses, old = run_steps(lib, 1, kg_dir, D, opt, params)
    lib.kge_set_option(b"counts_sort_blocked", 1)
    new_losses, new = run_steps(lib, 1, kg_dir, D, opt, params)
    assert old_losses == new_losses
    assert set(old) == set(new) and len(old) == (6 if opt == "Adam" else 2)
    for k in old:
        assert np.array_equal(bits(old[k]), bits(new[k])), k
    assert not np.array_equal(new["ent_embeddings"], params["ent_embeddings"])
