"""The host arithmetic of shared negatives across ranks, without a device: which global chunks a rank's slice of the batch meets
(train_paths.shared_chunk_span), that the ranks' slices partition the batch with every position in the chunk its GLOBAL position
names, and that a shared plan creates the entity table row-sharded where the unshared sparse-rows plan does."""
import pytest

from openkeonspark_amd import _lib, parallel, step_plan
from openkeonspark_amd.train_paths import shared_chunk_span


@pytest.mark.parametrize("P", [1, 4, 5, 127])
def test_chunk_span_against_a_loop(P):
    for first in range(0, 2 * P + 2):
        for n_pos in range(0, 3 * P + 1):
            chunks = sorted({p // P for p in range(first, first + n_pos)})
            c0, n_chunks = shared_chunk_span(first, n_pos, P)
            assert c0 == first // P
            assert n_chunks == len(chunks)
            if chunks:
                assert chunks == list(range(c0, c0 + n_chunks))


def test_chunk_span_refuses_nonsense():
    for bad in ((-1, 3, 4), (0, -1, 4), (0, 3, 0)):
        with pytest.raises(ValueError):
            shared_chunk_span(*bad)


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("batch", [5, 37, 1000])
def test_rank_slices_partition_the_batch_and_keep_global_chunks(batch, world):
    threads = 8
    for P in (1, 4, 5, 127):
        seen = []
        for g in range(world):
            lo, hi = parallel.thread_range(g, world, threads)
            first, n_pos = parallel.slice_positions(batch, threads, lo, hi)
            c0, n_chunks = shared_chunk_span(first, n_pos, P)
            for b in range(n_pos):
                p = first + b
                j = (first % P + b) // P          # the workgroup / row of the rank's candidate list that position lands in
                assert 0 <= j < n_chunks
                assert c0 + j == p // P           # ... is the chunk its global position names
                seen.append(p)
            if n_pos:
                assert c0 + n_chunks - 1 == (first + n_pos - 1) // P
        assert sorted(seen) == list(range(batch))      # every position on exactly one rank


@pytest.mark.parametrize("width,want", [(48, True), (200, True), (50, False)])
def test_a_shared_plan_shards_at_creation(width, want):
    plan = step_plan.plan(_lib.TRANSE, "SGD", None, True, True, 1003, 7, width, 600, 3, shared_chunk=5, negative_rel=0)
    assert plan.sparse_rows
    for world in (2, 8, 64):
        assert step_plan.shards_at_creation(plan, _lib.TRANSE, world, width) is want
    assert not step_plan.shards_at_creation(plan, _lib.TRANSE, 1, width)
    assert not step_plan.shards_at_creation(plan, _lib.TRANSE, 65, width)
