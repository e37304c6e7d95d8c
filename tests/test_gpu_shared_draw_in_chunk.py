"""kge_shared_negatives_draw_grouped_mixed: the lists of relation-grouped chunks with K in-chunk candidates beside the N drawn
ones (include/kge_mi355.h, "In-chunk candidates").  The drawn columns are held to kge_shared_negatives_draw_grouped's own output,
bit for bit; the in-chunk columns to the definition with its hashes written out here: the side of column k, the rotation of the
chunk (low key byte 64), the gather from h2 / t2, the -1 past the chunk's length, and the mask -- the corrupted triple is a
training triple, or the candidate is the entity it replaces.

The graph (E = 61) has, in relation 0, every triple of {1, 2, 3} x {10, 11, 12, 13}: a chunk of that relation holds tails that are
known tails of its other heads, so the lookup masks in-chunk pairs that the equality rule does not.  Batch position 0 is (5, 6, 0),
NOT a training triple: only the equality rule masks it against itself.  From 8 positives on, two relation ids lie outside the
table (the trailing run: no in-chunk candidate)."""
import numpy as np
import pytest

import shared_neg_ref as ref
from openkeonspark_amd.train_paths import shared_chunk_cap, shared_in_chunk_candidates, shared_relation_chunks

pytestmark = pytest.mark.gpu

E = 61
SEED = 0xC0FFEE12345
LONER = (5, 6, 0)
BLOCK_H, BLOCK_T = (1, 2, 3), (10, 11, 12, 13)


def graph(R):
    rng = np.random.default_rng(100 + R)
    n = 700
    h = rng.integers(0, E, n); r = rng.integers(0, R, n)
    t = (h + 1 + rng.integers(0, E - 1, n)) % E
    keep = ~((h == LONER[0]) & (t == LONER[1]) & (r == LONER[2]))
    bh, bt = np.meshgrid(BLOCK_H, BLOCK_T, indexing="ij")
    h = np.r_[h[keep], bh.ravel()]; t = np.r_[t[keep], bt.ravel()]; r = np.r_[r[keep], np.zeros(bh.size, dtype=np.int64)]
    return h.astype(np.int64), t.astype(np.int64), r.astype(np.int64)


def type_lists(R):
    """CSR head and tail lists: relation 0 has none (the untyped draw), the others a random third of the entities."""
    rng = np.random.default_rng(200 + R)
    lists = [[[] if k == 0 else sorted(rng.choice(E, E // 3, replace=False).tolist()) for k in range(R)] for _ in range(2)]
    out = ()
    for side in lists:
        out += (np.cumsum([0] + [len(x) for x in side]).astype(np.int64), np.array([v for x in side for v in x], dtype=np.int64))
    return out


def engine(R, bern):
    import openkeonspark_amd as ok
    con = ok.Config()
    con.set_work_threads(1); con.set_bern(bern)
    con.init_from_arrays(E, R, *graph(R))
    empty = (np.zeros(0, np.int64),) * 3
    con.init_evaluation_from_arrays(empty, empty, type_lists=type_lists(R))
    return con


def bern_table(con, R):
    out = np.zeros(R, np.float32)
    assert con.lib.kge_index_copy(b"bern_prob", out.ctypes.data, out.nbytes) == out.nbytes
    return out


def batch(R, n_pos, rng):
    gh, gt, gr = graph(R)
    pick = rng.integers(0, len(gh), n_pos)
    pick[: n_pos // 3] = len(gh) - 1 - rng.integers(0, len(BLOCK_H) * len(BLOCK_T), n_pos // 3)      # a third from the block of relation 0
    h, t, r = gh[pick].copy(), gt[pick].copy(), gr[pick].copy()
    h[0], t[0], r[0] = LONER
    if n_pos >= 8:
        r[3], r[n_pos - 1] = -1, R
    return h, t, r


def device_lists(L, h2, t2, r2, chunks, N, K, typed, step, mixed=True):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    dh, dt, dr, dc = dev(h2), dev(t2), dev(r2), dev(chunks)
    cap, n_pos, Nt = len(chunks), len(h2), N + K
    cand = torch.full((cap + 1, Nt), -9, dtype=torch.int32, device="cuda")
    pair = torch.full((n_pos + 1, Nt), 77, dtype=torch.uint8, device="cuda")
    if mixed:
        rc = L.kge_shared_negatives_draw_grouped_mixed(dh.data_ptr(), dt.data_ptr(), dr.data_ptr(), n_pos, dc.data_ptr(), cap, N, K, typed, SEED,
                                                       step, cand.data_ptr(), pair.data_ptr(), None)
    else:
        assert K == 0
        rc = L.kge_shared_negatives_draw_grouped(dh.data_ptr(), dt.data_ptr(), dr.data_ptr(), n_pos, dc.data_ptr(), cap, N, typed, SEED, step,
                                                 cand.data_ptr(), pair.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    cand, pair = cand.cpu().numpy(), pair.cpu().numpy()
    assert (cand[cap] == -9).all() and (pair[n_pos] == 77).all()      # nothing past the cap or the batch
    return cand[:cap], pair[:n_pos]


def in_chunk_definition(h2, t2, r2, chunks, n_chunks, N, K, R, bern_prob, train, step):
    """(ids int32 [cap, K], pair uint8 [n_pos, K], the number of pairs masked by the lookup alone, by the equality rule alone) of
    the in-chunk columns, from the definition: every hash is written out here."""
    u64 = np.uint64
    S, G = u64(ref.step_key(SEED, step)), u64(ref.GAMMA)
    cap, n_pos = len(chunks), len(h2)
    ids = np.full((cap, K), -1, dtype=np.int32)
    pair = np.zeros((n_pos, K), dtype=np.uint8)
    by_lookup = by_equality = 0
    with np.errstate(over="ignore"):
        for j in range(n_chunks):
            first, n = int(chunks[j, 0]), int(chunks[j, 1])
            rho = int(r2[first])
            valid = 0 <= rho < R
            o = int(((ref.mix(S + (((u64(j) << u64(8)) | u64(64)) + u64(1)) * G) >> u64(32)) * u64(n)) >> u64(32))
            for i in range(K):
                k = N + i
                v = ((ref.mix(S + (((u64(j) << u64(8)) | u64(128) | u64(k)) + u64(1)) * G) >> u64(32)) * u64(1000)) >> u64(32)
                prob = bern_prob[rho] if (bern_prob is not None and valid) else np.float32(500.0)
                new_tail = bool(np.float32(int(v)) < np.float32(prob))
                cid = -1
                if i < n and valid:
                    q = first + (o + i) % n
                    cid = int(t2[q]) if new_tail else int(h2[q])
                ids[j, i] = cid
                for b in range(first, first + n):
                    own = cid == (int(t2[b]) if new_tail else int(h2[b]))
                    known = valid and cid >= 0 and ((int(h2[b]), cid, rho) if new_tail else (cid, int(t2[b]), rho)) in train
                    masked = cid < 0 or own or known
                    pair[b, i] = (0 if new_tail else 1) | (2 if masked else 0)
                    if cid >= 0:
                        by_lookup += int(known and not own)
                        by_equality += int(own and not known)
    return ids, pair, by_lookup, by_equality


@pytest.mark.parametrize("bern", [0, 1])
@pytest.mark.parametrize("R", [1, 4, 300])
def test_in_chunk_columns_equal_the_definition_and_drawn_columns_the_grouped_draw(R, bern):
    con = engine(R, bern)
    L = con.lib
    prob = bern_table(con, R) if bern else None
    if bern and R > 1:
        assert len(set(prob.tolist())) > 1
    train = set(zip(*[a.tolist() for a in graph(R)]))
    assert LONER not in train
    rng = np.random.default_rng(7 + R + bern)
    seen = dict(short=0, exact=0, long=0, lookup=0, equality=0, trailing=0, heads=0, tails=0)
    step = 0
    for n_pos in (1, 11, 257):
        h, t, r = batch(R, n_pos, rng)
        for P in (1, 2, 5, 64):
            perm, chunks, n_chunks = shared_relation_chunks(r, P, R)
            cap = len(chunks)
            assert cap == shared_chunk_cap(n_pos, P, R) > n_chunks
            h2, t2, r2 = h[perm], t[perm], r[perm]
            for N, K in ((1, 1), (3, 4), (25, 38), (1, 62)):
                step += 1
                where = (R, bern, n_pos, P, N, K)
                old_cand, old_pair = device_lists(L, h2, t2, r2, chunks, N, 0, 0, step, mixed=False)
                cand, pair = device_lists(L, h2, t2, r2, chunks, N, K, 0, step)
                # the drawn columns: the grouped draw's, bit for bit; K = 0: all of it
                assert np.array_equal(cand[:, :N], old_cand) and np.array_equal(pair[:, :N], old_pair), where
                zero_cand, zero_pair = device_lists(L, h2, t2, r2, chunks, N, 0, 0, step)
                assert np.array_equal(zero_cand, old_cand) and np.array_equal(zero_pair, old_pair), where
                # the in-chunk columns: the definition
                want_ids, want_pair, by_lookup, by_equality = in_chunk_definition(h2, t2, r2, chunks, n_chunks, N, K, R, prob, train, step)
                assert np.array_equal(cand[:, N:], want_ids), where
                assert np.array_equal(pair[:, N:], want_pair), where
                # ... whose ids and rotation the host statement gives too, from the device's own sides
                valid = (r2[chunks[:n_chunks, 0]] >= 0) & (r2[chunks[:n_chunks, 0]] < R)
                sides = pair[chunks[:n_chunks, 0]] & 1
                assert np.array_equal(shared_in_chunk_candidates(h2, t2, chunks, n_chunks, sides, N, K, SEED, step, valid=valid),
                                      cand[:n_chunks, N:]), where
                # properties, from the device's own lists
                assert (cand[n_chunks:] == -1).all()
                for j in range(n_chunks):
                    first, n = chunks[j]
                    rho = int(r2[first])
                    if not 0 <= rho < R:      # the trailing run: no in-chunk candidate, every such pair masked
                        assert (cand[j, N:] == -1).all() and ((pair[first:first + n, N:] & 2) == 2).all(), where
                        seen["trailing"] += 1
                        continue
                    assert (cand[j, N + min(K, n):] == -1).all() and (cand[j, N:N + min(K, n)] >= 0).all(), where
                    assert ((pair[first:first + n, N + min(K, n):] & 2) == 2).all(), where      # no candidate: masked
                    seen["short" if n < K else "exact" if n == K else "long"] += 1
                    for i in range(min(K, n)):
                        side = set((pair[first:first + n, N + i] & 1).tolist())
                        assert len(side) == 1
                        pool = (h2 if side.pop() else t2)[first:first + n]
                        assert int(cand[j, N + i]) in pool.tolist(), where
                seen["heads"] += int(((pair[:, N:] & 1) == 1).sum()); seen["tails"] += int(((pair[:, N:] & 1) == 0).sum())
                seen["lookup"] += by_lookup; seen["equality"] += by_equality
                # the positive that is no training triple meets itself in its own chunk whenever the rotation brings it up: masked
                b_own = int(np.nonzero(perm == 0)[0][0])
                j_own = int(np.nonzero((chunks[:n_chunks, 0] <= b_own) & (b_own < chunks[:n_chunks, 0] + chunks[:n_chunks, 1]))[0][0])
                for i in range(K):
                    new_head = pair[b_own, N + i] & 1
                    if cand[j_own, N + i] == (h2 if new_head else t2)[b_own]:
                        assert pair[b_own, N + i] & 2, where
                # typed candidates: the in-chunk columns do not consult the lists; the drawn ones are the typed grouped draw's
                typed_old = device_lists(L, h2, t2, r2, chunks, N, 0, 1, step, mixed=False)
                typed_cand, typed_pair = device_lists(L, h2, t2, r2, chunks, N, K, 1, step)
                assert np.array_equal(typed_cand[:, :N], typed_old[0]) and np.array_equal(typed_pair[:, :N], typed_old[1]), where
                assert np.array_equal(typed_cand[:, N:], cand[:, N:]) and np.array_equal(typed_pair[:, N:], pair[:, N:]), where
                if R > 1 and n_pos > 1 and N > 1:
                    assert not np.array_equal(typed_old[0], old_cand), where      # (the lists were used)
    assert seen["short"] > 0 and seen["long" if R < 300 else "short"] > 0 and seen["trailing"] > 0
    assert seen["lookup"] > 0 and seen["equality"] > 0 and seen["heads"] > 0 and seen["tails"] > 0
    if R == 1:
        assert seen["exact"] > 0


def test_refusals_name_the_limit():
    import torch
    from openkeonspark_amd import _lib
    con = engine(4, 0)
    L = con.lib
    z = torch.zeros(4 * 63, dtype=torch.int32, device="cuda")
    table = torch.tensor([[0, 4], [4, 0]], dtype=torch.int32, device="cuda")
    p = z.data_ptr()
    for N, K in ((0, 3), (1, -1), (1, 63), (25, 39), (64, 0)):
        assert L.kge_shared_negatives_draw_grouped_mixed(p, p, p, 4, table.data_ptr(), 2, N, K, 0, 0, 0, p, p, None) < 0
        assert "N + K <= 63" in _lib.last_error(L)
    assert L.kge_shared_negatives_draw_grouped_mixed(p, p, p, 4, table.data_ptr(), 2, 1, 62, 0, 0, 0, p, p, None) == 0
    torch.cuda.synchronize()
