"""kge_shared_negatives_draw_grouped: the candidates, their sides and the masks of relation-grouped chunks against numpy written from
the definition (include/kge_mi355.h, "Shared negatives on RELATION-GROUPED chunks"): the hashes are spelled out here with
shared_neg_ref.mix, the type lists are the ones handed to the engine, the mask is membership in the set of training triples.

The graph (E = 61, R = 4) holds the cases of the typed draw: relation 0 has no list (the untyped draw), relation 1's tail list has
ONE entity, the tail of a positive of the batch (every new-tail candidate of its chunk is that positive's own tail: masked),
relation 2's lists cover all entities, relation 3 has ordinary partial lists; a positive with a relation id outside the table
sits in the trailing run."""
import numpy as np
import pytest

import shared_neg_ref as ref
from openkeonspark_amd.train_paths import shared_chunk_cap, shared_relation_chunks

pytestmark = pytest.mark.gpu

E, R = 61, 4
SEED = 0xC0FFEE12345
OWN = (7, 33, 1)                      # (h, t, r): relation 1's tail list is [33]
HEAD_LISTS = [[], [2, 7, 11, 19, 40, 41, 60], list(range(E)), [0, 5, 9, 30, 59]]
TAIL_LISTS = [[], [33], list(range(E)), [1, 4, 8, 15, 16, 23, 42]]


def graph():
    rng = np.random.default_rng(21)
    n = 500
    h = rng.integers(0, E, n); r = rng.integers(0, R, n)
    t = (h + 1 + rng.integers(0, E - 1, n)) % E
    # relation 3: many triples inside its lists, so that typed candidates meet known triples; relation 1: the own-tail positive
    h3 = rng.choice(HEAD_LISTS[3], 60); t3 = rng.choice(TAIL_LISTS[3], 60)
    h = np.r_[h, h3, OWN[0], [OWN[0]] * 3]; t = np.r_[t, t3, OWN[1], [5, 6, 8]]; r = np.r_[r, np.full(60, 3), OWN[2], [1] * 3]
    return h.astype(np.int64), t.astype(np.int64), r.astype(np.int64)


def csr(lists):
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int64)
    return off, np.array([v for x in lists for v in x], dtype=np.int64)


def engine(bern, lists=True):
    import openkeonspark_amd as ok
    con = ok.Config()
    con.set_work_threads(1); con.set_bern(bern)
    con.init_from_arrays(E, R, *graph())
    empty = (np.zeros(0, np.int64),) * 3      # (an evaluation import also drops the lists an earlier engine of the process left)
    con.init_evaluation_from_arrays(empty, empty, type_lists=csr(HEAD_LISTS) + csr(TAIL_LISTS) if lists else None)
    return con


def bern_table(con):
    out = np.zeros(R, np.float32)
    assert con.lib.kge_index_copy(b"bern_prob", out.ctypes.data, out.nbytes) == out.nbytes
    return out


def batch(n_pos, rng):
    """Training triples (so that candidates equal to the replaced entity are masked), the own-tail positive among them, and two
    positives whose relation id lies outside the table."""
    gh, gt, gr = graph()
    pick = rng.integers(0, len(gh), n_pos)
    h, t, r = gh[pick].copy(), gt[pick].copy(), gr[pick].copy()
    h[0], t[0], r[0] = OWN
    if n_pos >= 8:
        r[3], r[n_pos - 1] = -1, R
    return h, t, r


def definition(h2, t2, r2, chunks, n_chunks, N, typed, bern_prob, step):
    """cand int32 [cap, N] (-1 in unused slots), pair uint8 [n_pos, N], and per (chunk, k) whether the typed list was used."""
    u64 = np.uint64
    S = u64(ref.step_key(SEED, step))
    G = u64(ref.GAMMA)
    train = set(zip(*[a.tolist() for a in graph()]))
    cap, n_pos = len(chunks), len(h2)
    cand = np.full((cap, N), -1, dtype=np.int32)
    pair = np.zeros((n_pos, N), dtype=np.uint8)
    from_list = np.zeros((cap, N), dtype=bool)
    with np.errstate(over="ignore"):
        for j in range(n_chunks):
            b0, n = int(chunks[j, 0]), int(chunks[j, 1])
            rho = int(r2[b0])
            valid = 0 <= rho < R
            for k in range(N):
                c = (u64(j) << u64(8)) | u64(k)
                v = ((ref.mix(S + ((c | u64(128)) + u64(1)) * G) >> u64(32)) * u64(1000)) >> u64(32)
                prob = bern_prob[rho] if (bern_prob is not None and valid) else np.float32(500.0)
                new_tail = bool(np.float32(int(v)) < np.float32(prob))
                u = ref.mix(S + (c + u64(1)) * G) >> u64(32)
                L = (TAIL_LISTS if new_tail else HEAD_LISTS)[rho] if (typed and valid) else []
                if len(L):
                    cid = sorted(set(L))[int((u * u64(len(set(L)))) >> u64(32))]
                    from_list[j, k] = True
                else:
                    cid = int((u * u64(E)) >> u64(32))
                cand[j, k] = cid
                for b in range(b0, b0 + n):
                    corrupted = (int(h2[b]), cid, rho) if new_tail else (cid, int(t2[b]), rho)
                    pair[b, k] = (0 if new_tail else 1) | (2 if (valid and corrupted in train) else 0)
    return cand, pair, from_list


def draw_on_device(L, h2, t2, r2, chunks, N, typed, step):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    dh, dt, dr, dc = dev(h2), dev(t2), dev(r2), dev(chunks)
    cap, n_pos = len(chunks), len(h2)
    cand = torch.full((cap + 1, N), -9, dtype=torch.int32, device="cuda")
    pair = torch.full((n_pos + 1, N), 77, dtype=torch.uint8, device="cuda")
    rc = L.kge_shared_negatives_draw_grouped(dh.data_ptr(), dt.data_ptr(), dr.data_ptr(), n_pos, dc.data_ptr(), cap, N, typed, SEED, step,
                                             cand.data_ptr(), pair.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    cand, pair = cand.cpu().numpy(), pair.cpu().numpy()
    assert (cand[cap] == -9).all() and (pair[n_pos] == 77).all()      # nothing past the cap or the batch
    return cand[:cap], pair[:n_pos]


@pytest.mark.parametrize("bern", [0, 1])
def test_candidates_sides_and_masks_equal_the_definition(bern):
    con = engine(bern)
    L = con.lib
    prob = bern_table(con) if bern else None
    if bern:
        assert len(set(prob.tolist())) > 1 and not (prob == 500.0).all()
    train = set(zip(*[a.tolist() for a in graph()]))
    rng = np.random.default_rng(40 + bern)
    own_masked = typed_from_list = fallback = 0
    for n_pos, P, N in [(60, 4, 5), (300, 127, 63), (9, 1, 1), (1, 2, 3)]:
        h, t, r = batch(n_pos, rng)
        perm, chunks, n_chunks = shared_relation_chunks(r, P, R)
        assert len(chunks) == shared_chunk_cap(n_pos, P, R) > n_chunks                # (unused slots exist: their candidates are -1)
        h2, t2, r2 = h[perm], t[perm], r[perm]
        for typed in (1, 0):
            for step in (0, 5):
                want_cand, want_pair, from_list = definition(h2, t2, r2, chunks, n_chunks, N, typed, prob, step)
                cand, pair = draw_on_device(L, h2, t2, r2, chunks, N, typed, step)
                where = (bern, n_pos, P, N, typed, step)
                assert np.array_equal(cand, want_cand), where
                assert np.array_equal(pair, want_pair), where
                # properties, from the device's own lists
                for j in range(n_chunks):
                    b0, n = chunks[j]
                    rho = int(r2[b0])
                    for k in range(N):
                        sides = set((pair[b0:b0 + n, k] & 1).tolist())
                        assert len(sides) == 1                                            # one side per candidate of a chunk
                        lst = (HEAD_LISTS if sides.pop() else TAIL_LISTS)[rho] if 0 <= rho < R else []
                        if typed and lst:
                            assert int(cand[j, k]) in lst, (where, j, k)
                            typed_from_list += 1
                        else:
                            fallback += 1
                    for b in range(b0, b0 + n):
                        for k in range(N):
                            c = int(cand[j, k])
                            tri = (c, int(t2[b]), rho) if pair[b, k] & 1 else (int(h2[b]), c, rho)
                            assert bool(pair[b, k] & 2) == (0 <= rho < R and tri in train), (where, b, k)
                if typed:
                    b_own = int(np.nonzero(perm == 0)[0][0])                              # the own-tail positive
                    j_own = int(np.nonzero((chunks[:n_chunks, 0] <= b_own) & (b_own < chunks[:n_chunks, 0] + chunks[:n_chunks, 1]))[0][0])
                    tails = (pair[b_own] & 1) == 0
                    assert (cand[j_own][tails] == OWN[1]).all() and ((pair[b_own][tails] & 2) == 2).all()
                    own_masked += int(tails.sum())
    assert own_masked > 0 and typed_from_list > 0 and fallback > 0


def test_the_table_of_the_ordering_stage_gives_the_same_lists():
    """order -> draw on the device, nothing crossing the host in between, against the definition."""
    import torch
    con = engine(1)
    L = con.lib
    prob = bern_table(con)
    h, t, r = batch(257, np.random.default_rng(8))
    P, N, step = 16, 7, 3
    perm, chunks, n_chunks = shared_relation_chunks(r, P, R)
    cap = len(chunks)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    dh, dt, dr = dev(h), dev(t), dev(r)
    dperm = torch.empty(257, dtype=torch.int32, device="cuda"); ids = torch.empty((3, 257), dtype=torch.int32, device="cuda")
    dchunks = torch.empty((cap, 2), dtype=torch.int32, device="cuda"); dn = torch.zeros(1, dtype=torch.int32, device="cuda")
    cand = torch.empty((cap, N), dtype=torch.int32, device="cuda"); pair = torch.empty((257, N), dtype=torch.uint8, device="cuda")
    assert L.kge_shared_order_by_relation(dh.data_ptr(), dt.data_ptr(), dr.data_ptr(), 257, P, dperm.data_ptr(), ids[0].data_ptr(),
                                          ids[1].data_ptr(), ids[2].data_ptr(), dchunks.data_ptr(), dn.data_ptr(), None) == 0
    assert L.kge_shared_negatives_draw_grouped(ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), 257, dchunks.data_ptr(), cap, N, 1,
                                               SEED, step, cand.data_ptr(), pair.data_ptr(), None) == 0
    torch.cuda.synchronize()
    want_cand, want_pair, _ = definition(h[perm], t[perm], r[perm], chunks, n_chunks, N, 1, prob, step)
    assert int(dn.item()) == n_chunks
    assert np.array_equal(cand.cpu().numpy(), want_cand) and np.array_equal(pair.cpu().numpy(), want_pair)


def test_typed_without_lists_is_the_engines_own_error():
    import torch
    from openkeonspark_amd import _lib
    con = engine(0, lists=False)
    L = con.lib
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    table = torch.tensor([[0, 4], [4, 0]], dtype=torch.int32, device="cuda")
    p = z.data_ptr()
    assert L.kge_shared_negatives_draw_grouped(p, p, p, 4, table.data_ptr(), 2, 3, 1, 0, 0, p, p, None) < 0
    assert "type-constrained sampling" in _lib.last_error(L) and "no type file imported" in _lib.last_error(L)
    assert L.kge_shared_negatives_draw_grouped(p, p, p, 4, table.data_ptr(), 2, 3, 0, 0, 0, p, p, None) == 0      # untyped: fine
    torch.cuda.synchronize()
    for N in (0, 64):
        assert L.kge_shared_negatives_draw_grouped(p, p, p, 4, table.data_ptr(), 2, N, 0, 0, 0, p, p, None) < 0
        assert "63" in _lib.last_error(L)
