"""Shared negatives on relation-grouped chunks, the host side (Config.set_shared_negatives(..., by_relation=True)): the numpy
statement of the order and the chunk table against a brute-force loop, the bound on the chunk count, plans and refusals, the
checkpoint record of the two new fields, and the combination with type-constrained sampling that the feature exists for.
No GPU."""
import types

import numpy as np
import pytest

from openkeonspark_amd import KgeError, step_plan, train_paths
from openkeonspark_amd import distribute_training as dt
from test_step_plan import TRANSE, TRANSH

BASE = dict(model_id=TRANSE, opt_method="SGD", sparse_rows=None, use_counts=True, counts_supported=1, ent_total=993, rel_total=7,
            width=64, batch_size=128, n_neg=25, shared_chunk=64, negative_rel=0)


def brute_force(r, P, R):
    """The definition, one position at a time: positions in stable relation order, a new chunk at a new relation or after P."""
    key = [x if 0 <= x < R else R for x in r]
    perm = [b for k in range(R + 1) for b in range(len(r)) if key[b] == k]
    chunks = []
    for b, p in enumerate(perm):
        if b and key[perm[b - 1]] == key[p] and chunks[-1][1] < P:
            chunks[-1][1] += 1
        else:
            chunks.append([b, 1])
    return perm, chunks


def cases():
    rng = np.random.default_rng(3)
    out = []
    for n_pos, R, P in [(1, 1, 1), (11, 4, 2), (11, 4, 127), (257, 4, 64), (257, 300, 2), (300, 300, 1), (97, 1, 5), (64, 4, 64)]:
        out.append((rng.integers(0, R, n_pos), P, R))
        out.append((rng.integers(-1, R + 1, n_pos), P, R))      # ids of -1 and rel_total: the trailing run
    out.append((np.arange(300), 7, 300))                          # every position its own relation
    out.append((np.arange(300)[::-1].copy(), 7, 300))
    P = 5                                                         # runs of length 0 (relation 1), 1, P and P + 1
    out.append((np.array([0] + [2] * P + [3] * (P + 1))[rng.permutation(2 * P + 2)], P, 4))
    out.append((np.zeros(0, dtype=np.int64), 3, 4))
    return out


@pytest.mark.parametrize("r,P,R", cases())
def test_relation_chunks_equal_the_brute_force_loop(r, P, R):
    perm, chunks, n_chunks = train_paths.shared_relation_chunks(r, P, R)
    want_perm, want_chunks = brute_force([int(x) for x in r], P, R)
    cap = train_paths.shared_chunk_cap(len(r), P, R)
    assert perm.dtype == np.int32 and chunks.dtype == np.int32 and chunks.shape == (cap, 2)
    assert perm.tolist() == want_perm
    assert n_chunks == len(want_chunks) <= cap
    assert chunks[:n_chunks].tolist() == want_chunks
    assert (chunks[n_chunks:, 1] == 0).all() and (chunks[n_chunks:, 0] == len(r)).all()
    # the chunks partition the sorted positions, none is longer than P and none crosses a relation boundary
    assert chunks[:n_chunks, 1].sum() == len(r) and (chunks[:n_chunks, 1] <= P).all() and (chunks[:n_chunks, 1] >= 1).all()
    key = np.where((r >= 0) & (r < R), r, R)[perm]
    for b0, n in chunks[:n_chunks]:
        assert len(set(key[b0:b0 + n].tolist())) == 1


def test_the_chunk_count_stays_within_the_cap():
    """n_chunks <= cap = ceil(n_pos / P) + min(rel_total + 1, n_pos).  The second term counts the runs, each of which may end in
    one short piece, and it is reached exactly when every positive has its own relation: then n_chunks = n_pos = min(rel_total + 1,
    n_pos) = cap - ceil(n_pos / P).  (The sum itself is reached only by the empty batch: ceil(n_pos / P) >= 1 otherwise.)"""
    from openkeonspark_amd import _lib
    L = _lib.lib()
    for n_pos, P, R in [(1, 1, 1), (11, 2, 4), (257, 64, 300), (4099, 127, 300), (300, 7, 300), (299, 1, 298), (0, 3, 4)]:
        cap = train_paths.shared_chunk_cap(n_pos, P, R)
        assert cap == -(-n_pos // P) + min(R + 1, n_pos) == L.kge_shared_chunk_cap(n_pos, P, R)
    for P in (1, 2, 127):
        for r, R in ((np.arange(300), 300), (np.arange(300), 299), (np.arange(300)[::-1].copy(), 300)):      # (id 299 of 299: the trailing run)
            n_chunks = train_paths.shared_relation_chunks(r, P, R)[2]
            cap = train_paths.shared_chunk_cap(300, P, R)
            assert n_chunks == 300 == min(R + 1, 300) == cap - -(-300 // P)
    assert train_paths.shared_relation_chunks(np.zeros(0, dtype=np.int64), 3, 4)[2] == 0 == train_paths.shared_chunk_cap(0, 3, 4)
    # the worst case of short pieces: runs of P + 1 give two chunks each, still within the cap
    r = np.repeat(np.arange(4), 3)
    assert train_paths.shared_relation_chunks(r, 2, 4)[2] == 8 <= train_paths.shared_chunk_cap(12, 2, 4) == 6 + 5
    rng = np.random.default_rng(11)
    for _ in range(200):
        n_pos, R, P = int(rng.integers(1, 400)), int(rng.integers(1, 50)), int(rng.integers(1, 128))
        assert train_paths.shared_relation_chunks(rng.integers(-1, R + 1, n_pos), P, R)[2] <= train_paths.shared_chunk_cap(n_pos, P, R)
    with pytest.raises(ValueError):
        train_paths.shared_chunk_cap(5, 0, 3)
    assert L.kge_shared_chunk_cap(5, 0, 3) < 0


def test_plans_and_refusals():
    p = step_plan.plan(**dict(BASE, by_relation=True, typed=True))
    assert p.use_counts and p.sparse_rows and not p.sparse_inplace
    assert step_plan.plan(**dict(BASE, by_relation=True)) == step_plan.plan(**BASE) == step_plan.plan(**dict(BASE, by_relation=False, typed=False))
    with pytest.raises(KgeError) as exc:
        step_plan.plan(**dict(BASE, typed=True))
    for w in ("type-constrained", "by_relation", "typed candidates are not built"):
        assert w in str(exc.value)
    # every other refusal as worded, grouped or not
    for change, word in ((dict(opt_method="Adam"), "the dense count image has no entrance for shared records yet"),
                         (dict(model_id=TRANSH, counts_supported=0), "TransE only"), (dict(shared_chunk=128), "got 128"),
                         (dict(n_neg=26, negative_rel=1), "negative_rel must be 0"), (dict(n_neg=64, counts_supported=0), "got 64"),
                         (dict(use_counts=False), "sign-count")):
        for grouped in (dict(), dict(by_relation=True, typed=True)):
            with pytest.raises(KgeError, match=word):
                step_plan.plan(**dict(BASE, **change, **grouped))
    # with the option off the two arguments change nothing
    off = dict(BASE, shared_chunk=0)
    assert step_plan.plan(**off) == step_plan.plan(**dict(off, by_relation=True, typed=True))


def test_typed_sampling_and_grouped_shared_negatives_combine_in_either_order():
    """The test that fails without the feature: both calls raised "typed candidates are not built"."""
    import openkeonspark_amd as ok
    a = ok.Config()
    a.set_type_constrained_sampling(True)
    a.set_shared_negatives(8, by_relation=True)
    assert (a._shared_chunk, a._shared_by_relation, a.type_constrained_sampling) == (8, True, True)
    b = ok.Config()
    b.set_shared_negatives(8, seed=7, by_relation=True)
    b.set_type_constrained_sampling(True)
    assert (b._shared_chunk, b._shared_seed, b._shared_by_relation, b.type_constrained_sampling) == (8, 7, True, True)
    # without by_relation the two refusals stay, and name it
    c = ok.Config()
    c.set_type_constrained_sampling(True)
    with pytest.raises(KgeError, match="type-constrained") as exc:
        c.set_shared_negatives(8)
    assert "by_relation" in str(exc.value)
    d = ok.Config()
    d.set_shared_negatives(8)
    with pytest.raises(KgeError, match="type-constrained") as exc:
        d.set_type_constrained_sampling(True)
    assert "by_relation" in str(exc.value)
    # going back to position chunks while typed sampling is on is the same refusal; chunk = 0 forgets by_relation
    with pytest.raises(KgeError, match="by_relation"):
        a.set_shared_negatives(8)
    a.set_shared_negatives(0, by_relation=True)
    assert (a._shared_chunk, a._shared_by_relation) == (0, False)


def test_more_than_one_rank_is_refused_with_the_reason():
    import openkeonspark_amd as ok
    con = ok.Config()
    con.set_dimension(32)
    con.set_shared_negatives(8, by_relation=True)
    con.world_size = 2
    with pytest.raises(KgeError, match="one rank only") as exc:
        con._refuse_shared_ranks()
    assert "global order" in str(exc.value)
    con.world_size = 1
    con._refuse_shared_ranks()


def stub(chunk, seed=0, by_relation=False, typed=False):
    return types.SimpleNamespace(_shared_chunk=chunk, _shared_seed=seed, _shared_by_relation=by_relation, type_constrained_sampling=typed)


def test_checkpoint_record_round_trip(tmp_path):
    runs = [stub(0), stub(16, 5), stub(16, 5, True), stub(16, 5, True, True), stub(16, 6, True, True)]
    records = [dt.shared_negatives_record(c) for c in runs]
    assert [r.tolist() for r in records] == [[0, 0], [16, 5], [16, 5, 1, 0], [16, 5, 1, 1], [16, 6, 1, 1]]
    assert all(r.dtype == np.uint64 for r in records)
    for i, rec in enumerate(records):
        path = str(tmp_path / ("c%d.npz" % i))
        np.savez(path, shared_negatives=rec)
        z = dict(np.load(path).items())
        for k, run in enumerate(runs):
            if k == i:
                dt.check_shared_negatives_record(z, run)
            else:
                with pytest.raises(KgeError, match="shared negatives") as exc:
                    dt.check_shared_negatives_record(z, run)
                grouped = bool(runs[i]._shared_by_relation or run._shared_by_relation)      # (chunks by position on both sides: the older wording)
                assert ("--shared_negatives_by_relation" in str(exc.value)) == grouped
                assert ("(chunk, seed) = " in str(exc.value)) == (not grouped)
    # a checkpoint without the fields -- or without the record -- means False for both
    dt.check_shared_negatives_record({"shared_negatives": np.array([16, 5], dtype=np.uint64)}, stub(16, 5))
    dt.check_shared_negatives_record({}, stub(0))
    with pytest.raises(KgeError):
        dt.check_shared_negatives_record({"shared_negatives": np.array([16, 5], dtype=np.uint64)}, stub(16, 5, True))
    with pytest.raises(KgeError):
        dt.check_shared_negatives_record({}, stub(16, 5, True, True))
    # typed sampling without relation-grouped chunks cannot be configured, and is not recorded as typed candidates
    assert dt.shared_negatives_record(stub(16, 5, False, True)).tolist() == [16, 5]


def test_the_trainer_has_the_flag():
    argv = dt.parse_args(["--shared_negatives_chunk", "8", "--shared_negatives_by_relation", "1"])
    assert argv.shared_negatives_by_relation == 1 and argv.shared_negatives_chunk == 8
    assert dt.parse_args([]).shared_negatives_by_relation == 0
