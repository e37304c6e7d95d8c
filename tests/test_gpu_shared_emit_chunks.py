"""kge_transe_emit_records_shared_chunks alone: hand-made candidate / pair lists and hand-made CHUNK TABLES on the lattice tables of
tests/test_gpu_shared_emit.py (no sign and no hinge depends on fp32 summation order, asserted in fp64 before the device is
looked at), against an fp64 restatement of the definition that takes a chunk table.  Keys, reduced rows and int32 counts are
exact, the loss is within 1e-5.  A table that states fixed chunks of P must give kge_transe_emit_records_shared's records, keys
and loss bit for bit."""
import ctypes

import numpy as np
import pytest

import shared_neg_ref as ref
from test_gpu_shared_emit import E, MARGIN, R, SHAPES, check_conditions, desc_for, lattice_tables, reduce_on_device, run_shared

pytestmark = pytest.mark.gpu

DIMS = [4, 50, 200, 260]


def forward_chunks(ent, rel, h, t, r, cand, pair, chunks, margin, denom):
    """shared_neg_ref.forward with chunk j = the sorted positions [chunks[j][0], + chunks[j][1]); a slot of length 0 has no
    record.  3 n_pos + cap N records."""
    ent = np.asarray(ent, dtype=np.float64); rel = np.asarray(rel, dtype=np.float64)
    n_ent, D = ent.shape
    n_pos, N = pair.shape
    cap = len(chunks)
    H, T, Rn = ref.l2n(ent[h]), ref.l2n(ent[t]), ref.l2n(rel[r])
    ep = H + Rn - T
    p_score = np.abs(ep).sum(-1)
    sp = np.sign(ep).astype(np.int64)
    keys = np.full(3 * n_pos + cap * N, -1, dtype=np.int64)
    recs = np.zeros((3 * n_pos + cap * N, D), dtype=np.int64)
    active = np.zeros((n_pos, N), dtype=bool)
    loss, min_kink, min_sign = 0.0, np.inf, np.inf
    scored = np.zeros(n_pos, dtype=bool)
    for j, (lo, n) in enumerate(chunks):
        if n == 0:
            continue
        hi = lo + n
        c = cand[j].astype(np.int64)
        ok = (c >= 0) & (c < n_ent)
        C = ref.l2n(ent[np.where(ok, c, 0)])
        pb = pair[lo:hi]
        live = ((pb & 2) == 0) & ok[None, :]
        head = (pb & 1) == 1
        e = np.where(head[:, :, None], C[None, :, :] + (Rn[lo:hi] - T[lo:hi])[:, None, :], (H[lo:hi] + Rn[lo:hi])[:, None, :] - C[None, :, :])
        v = p_score[lo:hi, None] - np.abs(e).sum(-1) + margin
        act = live & (v >= 0)
        active[lo:hi] = act
        loss += float(v[act].sum())
        if live.any():
            min_kink = min(min_kink, float(np.abs(v[live]).min()))
            min_sign = min(min_sign, float(np.abs(e[live]).min()))
        scored[lo:hi] = live.any(1)
        s = np.sign(e).astype(np.int64) * act[:, :, None]
        base = 3 * n_pos + j * N
        recs[base:base + N] = np.where(head[:, :, None], -s, s).sum(0)
        keys[base:base + N] = np.where(act.any(0), c, -1)
        cnt = act.sum(1)[:, None]
        recs[lo:hi] = -(s * ~head[:, :, None]).sum(1) + cnt * sp[lo:hi]
        recs[n_pos + lo:n_pos + hi] = (s * head[:, :, None]).sum(1) - cnt * sp[lo:hi]
        recs[2 * n_pos + lo:2 * n_pos + hi] = -s.sum(1) + cnt * sp[lo:hi]
    for slot, ids in enumerate((np.asarray(h, dtype=np.int64), np.asarray(t, dtype=np.int64), np.asarray(r, dtype=np.int64) + n_ent)):
        blk = slice(slot * n_pos, (slot + 1) * n_pos)
        keys[blk] = np.where(np.abs(recs[blk]).sum(1) > 0, ids, -1)
    if scored.any():
        min_sign = min(min_sign, float(np.abs(ep[scored]).min()))
    return dict(keys=keys, records=recs, loss=loss / denom, min_kink=min_kink, min_sign=min_sign, active=active)


def table_of(lens, empty=2):
    """Contiguous chunks of the given lengths, then `empty` slots of length 0 (first position n_pos, as the ordering stage writes)."""
    starts = np.cumsum([0] + list(lens))
    n_pos = int(starts[-1])
    return np.array([[s, n] for s, n in zip(starts[:-1], lens)] + [[n_pos, 0]] * empty, dtype=np.int32), n_pos


def make_lists(n_pos, cap, N, seed, mask=True):
    """Positives and lists with a repeated candidate, a positive's own head as a new tail, ids outside the table, a positive with
    every pair masked and random masks (where the shape has room); the rows of `cand` beyond the used slots hold valid ids that
    must not be read as candidates."""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, E, n_pos); t = (h + 1 + rng.integers(0, E - 1, n_pos)) % E; r = rng.integers(0, R, n_pos)
    cand = rng.integers(0, E, (cap, N)).astype(np.int32)
    pair = rng.integers(0, 2, (n_pos, N)).astype(np.uint8)
    cand[0, 0] = h[0]; pair[0, 0] = 0
    if N >= 2:
        cand[0, 1] = cand[0, 0]
    if N >= 3 and mask:
        cand[1 % cap, 2] = E + 3
        cand[0, N - 1] = -1
    if mask:
        if n_pos >= 3:
            pair[n_pos // 2] |= 2
        pair |= (rng.random((n_pos, N)) < 0.1).astype(np.uint8) << 1
    return h.astype(np.int32), t.astype(np.int32), r.astype(np.int32), cand, pair


def run_chunks(L, desc, ent, rel, h, t, r, cand, pair, chunks, stride, denom):
    import torch
    n_pos, N = pair.shape
    cap = len(chunks)
    M = 3 * n_pos + cap * N
    dw = int(L.kge_transe_record_dwords(ctypes.byref(desc)))
    dev = lambda a, n=None: torch.from_numpy(np.concatenate([a, np.zeros((n or len(a)) - len(a), a.dtype)])).cuda()
    dh, dt, dr = dev(h, stride), dev(t, stride), dev(r, stride)
    dc, dp, dtab = torch.from_numpy(cand).cuda(), torch.from_numpy(pair).cuda(), torch.from_numpy(np.ascontiguousarray(chunks)).cuda()
    rec = torch.full((M + 1, dw), 0x55, dtype=torch.int32, device="cuda")
    dst = torch.full((M + 1,), -7, dtype=torch.int32, device="cuda")
    loss = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    rc = L.kge_transe_emit_records_shared_chunks(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), dh.data_ptr(), dt.data_ptr(), dr.data_ptr(),
                                                 n_pos, stride, dtab.data_ptr(), cap, dc.data_ptr(), N, dp.data_ptr(), denom, rec.data_ptr(),
                                                 dst.data_ptr(), loss.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(dst[M].item()) == -7 and (rec[M] == 0x55).all()      # nothing past the last record
    return rec[:M], dst[:M], loss


@pytest.fixture(scope="module")
def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("P,N", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_records_equal_the_definition(lib, D, P, N):
    """Chunks of length P, 1, P - 1, P, 1 (P - 1 where it is a length), then two empty slots."""
    import torch
    lens = [P, 1] + ([P - 1] if P >= 2 else []) + [P, 1]
    chunks, n_pos = table_of(lens)
    cap = len(chunks)
    ent_h, rel_h = lattice_tables(D, 19 * D + P)
    h, t, r, cand, pair = make_lists(n_pos, cap, N, 2000 * D + 10 * P + N)
    denom = n_pos * N
    want = forward_chunks(ent_h, rel_h, h, t, r, cand, pair, chunks, MARGIN, denom)
    check_conditions(want)
    desc = desc_for(D, MARGIN)
    ent = torch.from_numpy(ent_h).cuda(); rel = torch.from_numpy(rel_h).cuda()
    rec, dst, loss = run_chunks(lib, desc, ent, rel, h, t, r, cand, pair, chunks, n_pos + 5, denom)
    loss = float(loss.item())
    print("D %d P %d N %d n_pos %d cap %d: active %d of %d pairs, loss %.6f (fp64 %.6f), min kink %.2e, min sign %.2e"
          % (D, P, N, n_pos, cap, int(want["active"].sum()), n_pos * N, loss, want["loss"], want["min_kink"], want["min_sign"]))
    assert n_pos * N < 20 or want["active"].any()
    keys = dst.cpu().numpy().astype(np.int64)
    assert np.array_equal(keys, want["keys"])
    assert (keys[3 * n_pos + (cap - 2) * N:] == -1).all()           # the empty slots' candidate keys
    rows, counts = reduce_on_device(lib, desc, rec.contiguous(), dst.contiguous(), D)
    want_rows, want_counts = ref.reduce(want["keys"], want["records"])
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(counts, want_counts)
    assert abs(loss - want["loss"]) <= 1e-5 * abs(want["loss"])


@pytest.mark.parametrize("P,N", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_a_table_of_fixed_chunks_is_the_fixed_chunk_kernel_bit_for_bit(lib, D, P, N):
    import torch
    n_pos = 2 * P + 3
    n_chunks = -(-n_pos // P)
    fixed = np.array([[j * P, min(P, n_pos - j * P)] for j in range(n_chunks)], dtype=np.int32)
    ent_h, rel_h = lattice_tables(D, 23 * D + N)
    h, t, r, cand, pair = make_lists(n_pos, n_chunks + 2, N, 3000 * D + 10 * P + N)
    denom = n_pos * N
    desc = desc_for(D, MARGIN)
    ent = torch.from_numpy(ent_h).cuda(); rel = torch.from_numpy(rel_h).cuda()
    rec0, dst0, loss0 = run_shared(lib, desc, ent, rel, h, t, r, cand[:n_chunks], pair, P, n_pos + 2, denom)
    loss0_bits = np.float32(loss0).view(np.uint32)
    M = 3 * n_pos + n_chunks * N
    for empty in (0, 2):
        table = np.concatenate([fixed, np.array([[n_pos, 0]] * empty, dtype=np.int32).reshape(-1, 2)])
        rec, dst, loss = run_chunks(lib, desc, ent, rel, h, t, r, cand[:n_chunks + empty], pair, table, n_pos + 2, denom)
        assert torch.equal(dst[:M], dst0) and torch.equal(rec[:M], rec0)
        assert (dst[M:] == -1).all()
        assert loss.cpu().numpy().view(np.uint32)[0] == loss0_bits
    assert (dst0 >= 0).any()


def test_refusals(lib):
    """emit_call's refusals, with their words; a missing table is a bad argument."""
    import torch
    from openkeonspark_amd import _lib
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    f = torch.zeros((E + R, 1024), dtype=torch.float32, device="cuda")
    table = torch.tensor([[0, 1]], dtype=torch.int32, device="cuda")

    def call(desc, N, tab=table.data_ptr(), cap=1):
        return lib.kge_transe_emit_records_shared_chunks(ctypes.byref(desc), f.data_ptr(), f.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                                         1, 1, tab, cap, z.data_ptr(), N, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(),
                                                         f.data_ptr(), None)

    for change, N, word in ((dict(model=1), 2, "TransE"), (dict(negative_rel=1), 2, "negative_rel"), ({}, 64, "63"),
                            (dict(ent_dim=516, rel_dim=516), 2, "512")):
        d = desc_for(8, 1.0)
        for k, v in change.items():
            setattr(d, k, v)
        assert call(d, N) == -4
        assert word in _lib.last_error(lib)
    assert call(desc_for(8, 1.0), 2, tab=None) < 0
    assert call(desc_for(8, 1.0), 2, cap=0) < 0
    assert call(desc_for(8, 1.0), 2) == 0
    torch.cuda.synchronize()
