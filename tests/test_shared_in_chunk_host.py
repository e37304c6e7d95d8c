"""In-chunk candidates of relation-grouped shared negatives, the host side (Config.set_shared_negatives(..., in_chunk=K);
include/kge_mi355.h, "In-chunk candidates"): the numpy statement of the rotation and the ids against a brute-force loop, the
refusals and their words, the plans, the checkpoint record's fifth field and the trainer's flag.  No GPU."""
import os
import types

import numpy as np
import pytest

import shared_neg_ref as ref
from conftest import GOLDEN
from openkeonspark_amd import KgeError, step_plan, train_paths
from openkeonspark_amd import distribute_training as dt
from openkeonspark_amd._lib import TRANSD, TRANSE, TRANSH, TRANSR

SEED = 0xC0FFEE12345


def brute_force(h2, t2, chunks, n_chunks, sides, K, seed, step):
    """The definition, one column at a time, with the hash spelled out."""
    u64 = np.uint64
    S, G = u64(ref.step_key(seed, step)), u64(ref.GAMMA)
    out = np.full((n_chunks, K), -1, dtype=np.int64)
    with np.errstate(over="ignore"):
        for j in range(n_chunks):
            first, n = int(chunks[j][0]), int(chunks[j][1])
            o = int(((ref.mix(S + (((u64(j) << u64(8)) | u64(64)) + u64(1)) * G) >> u64(32)) * u64(n)) >> u64(32))
            assert 0 <= o < n
            for i in range(min(K, n)):
                q = first + (o + i) % n
                out[j, i] = t2[q] if sides[j][i] == 0 else h2[q]
    return out


def test_the_numpy_statement_equals_the_brute_force_loop():
    """Chunks shorter than K, of exactly K and longer (whose rotation wraps: o + i passes the chunk's end), over several steps."""
    rng = np.random.default_rng(5)
    K, N, P = 4, 3, 9
    r = np.r_[np.zeros(2), np.ones(4), np.full(9, 2), np.full(9, 2), np.full(3, 2), np.full(1, 3)].astype(np.int64)[rng.permutation(28)]
    perm, chunks, n_chunks = train_paths.shared_relation_chunks(r, P, 4)
    assert sorted(chunks[:n_chunks, 1].tolist()) == [1, 2, 3, 4, 9, 9]      # short, exactly K, long
    h2, t2 = rng.permutation(1000)[:28], 1000 + rng.permutation(1000)[:28]     # (distinct ids; heads and tails tell themselves apart)
    wrapped = short = 0
    for step in range(6):
        sides = rng.integers(0, 2, (n_chunks, K)).astype(np.uint8)
        want = brute_force(h2, t2, chunks, n_chunks, sides, K, SEED, step)
        got = train_paths.shared_in_chunk_candidates(h2, t2, chunks, n_chunks, sides, N, K, SEED, step)
        assert got.dtype == np.int32 and got.shape == (n_chunks, K) and np.array_equal(got, want)
        # the N + K wide form reads its last K columns, whatever stands before them
        wide = np.concatenate([rng.integers(0, 2, (n_chunks, N)).astype(np.uint8), sides | 2], axis=1)
        assert np.array_equal(train_paths.shared_in_chunk_candidates(h2, t2, chunks, n_chunks, wide, N, K, SEED, step), want)
        for j in range(n_chunks):
            first, n = chunks[j]
            live = got[j][got[j] >= 0]
            assert len(live) == min(K, n) and (got[j, min(K, n):] == -1).all()
            short += int(n < K)
            # the ids are the chunk's own, at consecutive rotated positions: distinct positions, so with these distinct ids no repeats
            pos = [int(np.flatnonzero((t2 if s == 0 else h2) == c)[0]) for c, s in zip(live, sides[j])]
            assert all(first <= q < first + n for q in pos) and len(set(pos)) == len(pos)
            assert all((b - a) % n == 1 for a, b in zip(pos, pos[1:]))
            wrapped += int(any(b < a for a, b in zip(pos, pos[1:])))
    assert wrapped > 0 and short > 0
    # the trailing run: a chunk marked as not valid has no in-chunk candidate
    valid = np.ones(n_chunks, dtype=bool); valid[1] = False
    got = train_paths.shared_in_chunk_candidates(h2, t2, chunks, n_chunks, sides, N, K, SEED, 5, valid=valid)
    assert (got[1] == -1).all() and np.array_equal(np.delete(got, 1, 0), np.delete(want, 1, 0))
    # no chunk, no column
    assert train_paths.shared_in_chunk_candidates([], [], np.zeros((0, 2)), 0, np.zeros((0, K)), N, K, SEED, 0).shape == (0, K)
    assert train_paths.shared_in_chunk_candidates(h2, t2, chunks, n_chunks, np.zeros((n_chunks, 0)), N, 0, SEED, 0).shape == (n_chunks, 0)
    with pytest.raises(ValueError, match="sides"):
        train_paths.shared_in_chunk_candidates(h2, t2, chunks, n_chunks, np.zeros((n_chunks, K + 1)), N, K, SEED, 0)


def test_the_rotation_key_is_no_candidate_key_and_no_side_key():
    """Candidate keys have a low byte of at most 62, side keys of at least 128: 64 is free, for every chunk."""
    assert all((k & 0xFF) != 64 and ((128 | k) & 0xFF) != 64 for k in range(63))


BASE = dict(model_id=TRANSE, opt_method="SGD", sparse_rows=None, use_counts=True, counts_supported=1, ent_total=993, rel_total=7,
            width=64, batch_size=128, n_neg=25, shared_chunk=64, negative_rel=0, by_relation=True)
MODELS = [(TRANSE, {}), (TRANSH, dict(counts_supported=0, shared_float_supported=1)),
          (TRANSD, dict(counts_supported=0, shared_transd_supported=1)), (TRANSR, dict(counts_supported=0, shared_transr_supported=1))]


@pytest.mark.parametrize("model_id,kw", MODELS)
@pytest.mark.parametrize("typed", [False, True])
def test_the_plan_is_the_plan_without_in_chunk_candidates(model_id, kw, typed):
    base = dict(BASE, model_id=model_id, typed=typed, **kw)
    for opt in ("SGD", "Adagrad") + (("LazyAdam",) if model_id != TRANSR else ("Adam",)):
        for K in (1, 12, 38):
            assert step_plan.plan(**dict(base, opt_method=opt, in_chunk=K)) == step_plan.plan(**dict(base, opt_method=opt)) \
                == step_plan.plan(**dict(base, opt_method=opt, in_chunk=0))
    # with shared negatives off the argument changes nothing
    off = dict(base, shared_chunk=0, by_relation=False, typed=False)
    assert step_plan.plan(**off) == step_plan.plan(**dict(off, in_chunk=5))


@pytest.mark.parametrize("model_id,kw", MODELS)
def test_refusals_name_their_limit(model_id, kw):
    base = dict(BASE, model_id=model_id, **kw)
    with pytest.raises(KgeError, match="in-chunk candidates need chunks of one relation") as exc:
        step_plan.plan(**dict(base, model_id=TRANSE, counts_supported=1, by_relation=False, in_chunk=4))
    for w in ("by_relation=True", "no single side", "slice of another rank"):
        assert w in str(exc.value)
    with pytest.raises(KgeError, match="in_chunk .* must be 0 or more, got -1"):
        step_plan.plan(**dict(base, in_chunk=-1))
    with pytest.raises(KgeError, match=r"at most 63 per positive .* got 25 \+ 39") as exc:
        step_plan.plan(**dict(base, in_chunk=39))
    assert "int8" in str(exc.value)
    step_plan.plan(**dict(base, in_chunk=38))                       # 25 + 38 = 63: taken
    step_plan.plan(**dict(base, n_neg=1, in_chunk=62))
    # the existing refusals keep their words with the keyword present
    for change, word in ((dict(n_neg=64), "1 to 63 negatives per positive"), (dict(n_neg=0), "1 to 63 negatives per positive"),
                         (dict(shared_chunk=128), "1 to 127"), (dict(n_neg=26, negative_rel=1), "negative_rel must be 0")):
        with pytest.raises(KgeError, match=word):
            step_plan.plan(**dict(base, in_chunk=3, **change))


def test_the_config_keyword_and_its_refusals():
    import openkeonspark_amd as ok
    a = ok.Config()
    assert a._shared_in_chunk == 0
    a.set_shared_negatives(8, seed=3, by_relation=True, in_chunk=5)
    assert (a._shared_chunk, a._shared_seed, a._shared_by_relation, a._shared_in_chunk) == (8, 3, True, 5)
    a.set_shared_negatives(8, seed=3, by_relation=True)
    assert a._shared_in_chunk == 0                                  # the default is off
    with pytest.raises(KgeError, match="in-chunk candidates need chunks of one relation"):
        a.set_shared_negatives(8, in_chunk=5)
    with pytest.raises(KgeError, match="must be 0 or more"):
        a.set_shared_negatives(8, by_relation=True, in_chunk=-2)
    assert (a._shared_chunk, a._shared_by_relation, a._shared_in_chunk) == (8, True, 0)      # a refused call changes nothing
    a.set_shared_negatives(8, by_relation=True, in_chunk=5)
    a.set_shared_negatives(0, by_relation=True, in_chunk=5)         # chunk = 0 forgets it with everything else
    assert (a._shared_chunk, a._shared_by_relation, a._shared_in_chunk) == (0, False, 0)
    # more than one rank stays refused by the by-relation message that is there
    b = ok.Config()
    b.set_dimension(32)
    b.set_shared_negatives(8, by_relation=True, in_chunk=2)
    b.world_size = 2
    with pytest.raises(KgeError, match="one rank only") as exc:
        b._refuse_shared_ranks()
    assert "global order" in str(exc.value)


def stub(chunk, seed=0, by_relation=False, typed=False, in_chunk=None):
    s = types.SimpleNamespace(_shared_chunk=chunk, _shared_seed=seed, _shared_by_relation=by_relation, type_constrained_sampling=typed)
    if in_chunk is not None:
        s._shared_in_chunk = in_chunk
    return s


def test_checkpoint_record_has_four_fields_without_and_five_with(tmp_path):
    runs = [stub(16, 5, True), stub(16, 5, True, in_chunk=0), stub(16, 5, True, True, in_chunk=0), stub(16, 5, True, in_chunk=12),
            stub(16, 5, True, True, in_chunk=12), stub(16, 5, True, in_chunk=13)]
    records = [dt.shared_negatives_record(c).tolist() for c in runs]
    assert records == [[16, 5, 1, 0], [16, 5, 1, 0], [16, 5, 1, 1], [16, 5, 1, 0, 12], [16, 5, 1, 1, 12], [16, 5, 1, 0, 13]]
    assert dt.shared_negatives_record(stub(16, 5, in_chunk=0)).tolist() == [16, 5] and dt.shared_negatives_record(stub(0, in_chunk=0)).tolist() == [0, 0]
    assert dt.shared_negatives_record(runs[3]).dtype == np.uint64
    same = {0: (0, 1), 1: (0, 1), 2: (2,), 3: (3,), 4: (4,), 5: (5,)}
    for i, run_i in enumerate(runs):
        path = str(tmp_path / ("c%d.npz" % i))
        np.savez(path, shared_negatives=dt.shared_negatives_record(run_i))
        z = dict(np.load(path).items())
        for k, run in enumerate(runs):
            if k in same[i]:
                dt.check_shared_negatives_record(z, run)
                continue
            with pytest.raises(KgeError, match="shared negatives") as exc:
                dt.check_shared_negatives_record(z, run)
            only_k = records[i][:4] == records[k][:4]
            assert ("--shared_negatives_in_chunk" in str(exc.value)) == only_k
            if only_k:
                a, b = (records[i] + [0])[4], (records[k] + [0])[4]
                assert "%d in-chunk candidates" % a in str(exc.value) and "this run has %d" % b in str(exc.value)
    # a checkpoint from before the field, or without the record: K = 0
    old = {"shared_negatives": np.array([16, 5, 1, 0], dtype=np.uint64)}
    dt.check_shared_negatives_record(old, stub(16, 5, True, in_chunk=0))
    with pytest.raises(KgeError, match="--shared_negatives_in_chunk"):
        dt.check_shared_negatives_record(old, stub(16, 5, True, in_chunk=12))
    with pytest.raises(KgeError, match="shared negatives"):
        dt.check_shared_negatives_record({}, stub(16, 5, True, in_chunk=12))
    dt.check_shared_negatives_record({}, stub(0, in_chunk=0))


def test_the_flag_reaches_the_config():
    assert dt.parse_args([]).shared_negatives_in_chunk == 0
    base = ["--input_path", os.path.join(GOLDEN, "kg_tiny"), "--embedding_dimension", "8", "--n_mini_batches", "2", "--ent_neg_rate", "3",
            "--shared_negatives_chunk", "8", "--shared_negatives_seed", "9", "--shared_negatives_by_relation", "1"]
    argv = dt.parse_args(base + ["--shared_negatives_in_chunk", "4"])
    assert argv.shared_negatives_in_chunk == 4
    con = dt.get_conf(argv)
    assert (con._shared_chunk, con._shared_seed, con._shared_by_relation, con._shared_in_chunk, con.negative_ent) == (8, 9, True, 4, 3)
    assert dt.shared_negatives_record(con).tolist() == [8, 9, 1, 0, 4]
    assert dt.get_conf(dt.parse_args(base))._shared_in_chunk == 0
    with pytest.raises(KgeError, match="in-chunk candidates need chunks of one relation"):
        dt.get_conf(dt.parse_args(base[:-2] + ["--shared_negatives_in_chunk", "4"]))
