"""kge_transe_emit_records_shared alone, on hand-made candidate / pair lists, against the fp64 restatement of the definition
(tests/shared_neg_ref.py) and against the existing emit kernel on the expanded batch.

The comparison is EXACT on the integers.  The inputs are built so that no hinge decision and no sign depends on fp32 summation
order, and every test asserts that on the host in fp64 before it looks at the device:
  kink condition  no unmasked pair with |p - n + margin| < 1e-4
  sign condition  no element |h^ + r^ - t^| < 1e-5 in any scored triple
Random normal rows cannot meet the sign condition at these sizes (about 1e-4 of all elements of a width-512 row difference lie
within 1e-5 of zero), so the tables are drawn from a lattice: an entity row is a signed permutation of half ones and half threes,
a relation row is all +-0.07.  After l2 normalisation every entity element is +-1 / sqrt(5 D) or +-3 / sqrt(5 D) and every
relation element +-1 / sqrt(D), and no signed sum x + r - y of them is closer to zero than 0.105 / sqrt(D) (= 4.6e-3 at D = 512).
Signs and permutations are random, so scores, hinges and counts vary freely."""
import ctypes

import numpy as np
import pytest

import shared_neg_ref as ref

pytestmark = pytest.mark.gpu

E, R = 61, 5
MARGIN = 0.3217
DIMS = [4, 50, 200, 260, 512]
SHAPES = [(1, 1), (2, 63), (64, 25), (127, 2)]


def lattice_tables(D, seed):
    rng = np.random.default_rng(seed)
    mags = np.array([1.0] * (D - D // 2) + [3.0] * (D // 2))
    ent = np.stack([rng.permutation(mags) for _ in range(E)]) * rng.choice([-1.0, 1.0], (E, D)) * 0.1
    rel = rng.choice([-1.0, 1.0], (R, D)) * 0.07
    return ent.astype(np.float32), rel.astype(np.float32)


def make_lists(P, N, n_pos, seed, mask=True):
    """Positives and lists holding every case the kernel must get right (where the shape has room for it): a repeated candidate,
    the positive's own head as a new tail, another positive's entity of the same chunk, a positive with every pair masked, a chunk
    with every pair masked, an id outside the table."""
    rng = np.random.default_rng(seed)
    n_chunks = -(-n_pos // P)
    h = rng.integers(0, E, n_pos); t = (h + 1 + rng.integers(0, E - 1, n_pos)) % E; r = rng.integers(0, R, n_pos)
    cand = rng.integers(0, E, (n_chunks, N)).astype(np.int32)
    pair = rng.integers(0, 2, (n_pos, N)).astype(np.uint8)
    slots = [(j, k) for j in range(n_chunks) for k in range(N)]
    it = iter(slots)
    has = {}
    j, k = next(it); cand[j, k] = h[j * P]; pair[j * P, k] = 0; has["own_head"] = (j, k)       # (h, r, h): the head as the new tail
    if N >= 2:
        j, k = next(it); cand[j, k] = cand[j, 0] if k else cand[j, 1]; has["repeat"] = (j, k)
    nxt = next(it, None)
    if nxt and min(P, n_pos - nxt[0] * P) >= 2:
        j, k = nxt; cand[j, k] = t[j * P + 1]; has["other_positive"] = (j, k)
    nxt = next(it, None)
    if nxt and mask:
        j, k = nxt; cand[j, k] = E + 3; has["out_of_range"] = (j, k)
        nxt = next(it, None)
        if nxt:
            cand[nxt] = -1
    if mask:
        if n_pos >= 3:
            pair[n_pos // 2] |= 2; has["masked_positive"] = n_pos // 2
        if n_chunks >= 3:
            pair[P:2 * P] |= 2; has["masked_chunk"] = 1
        pair |= (rng.random((n_pos, N)) < 0.1).astype(np.uint8) << 1
    else:
        # the expanded batch must be sampler-shaped: a candidate may not be the entity it replaces
        c = cand[np.arange(n_pos) // P]
        same = np.where(pair & 1, c == h[:, None], c == t[:, None])
        for b, k in zip(*np.nonzero(same)):
            pair[b, k] ^= 1
        c = cand[np.arange(n_pos) // P]
        assert not np.where(pair & 1, c == h[:, None], c == t[:, None]).any()
    return h.astype(np.int32), t.astype(np.int32), r.astype(np.int32), cand, pair, has


def desc_for(D, margin):
    from openkeonspark_amd import _lib
    d = _lib.ModelDesc()
    d.model = 0; d.negative_rel = 0; d.ent_total = E; d.rel_total = R; d.ent_dim = D; d.rel_dim = D; d.margin = margin
    return d


def reduce_on_device(L, desc, rec, dst, D):
    import torch
    n = dst.numel()
    rows = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    counts = torch.zeros((n, D), dtype=torch.int32, device="cuda")
    n_rows = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.kge_transe_reduce_records(ctypes.byref(desc), rec.data_ptr(), dst.clone().data_ptr(), n, rows.data_ptr(), counts.data_ptr(),
                                       n_rows.data_ptr(), None) == 0
    torch.cuda.synchronize()
    m = int(n_rows.item())
    return rows[:m].cpu().numpy().astype(np.int64), counts[:m].cpu().numpy().astype(np.int64)


def run_shared(L, desc, ent, rel, h, t, r, cand, pair, P, stride, denom):
    import torch
    n_pos, N = pair.shape
    n_chunks = cand.shape[0]
    M = 3 * n_pos + n_chunks * N
    dw = int(L.kge_transe_record_dwords(ctypes.byref(desc)))
    dev = lambda a, n=None: torch.from_numpy(np.concatenate([a, np.zeros((n or len(a)) - len(a), a.dtype)])).cuda()
    dh, dt, dr = dev(h, stride), dev(t, stride), dev(r, stride)
    dc, dp = torch.from_numpy(cand).cuda(), torch.from_numpy(pair).cuda()
    rec = torch.full((M, dw), 0x55, dtype=torch.int32, device="cuda")
    dst = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    loss = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    rc = L.kge_transe_emit_records_shared(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), dh.data_ptr(), dt.data_ptr(), dr.data_ptr(),
                                          n_pos, stride, P, dc.data_ptr(), N, dp.data_ptr(), denom, rec.data_ptr(), dst.data_ptr(),
                                          loss.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return rec, dst, float(loss.item())


def check_conditions(want):
    assert want["min_kink"] >= 1e-4, want["min_kink"]
    assert want["min_sign"] >= 1e-5, want["min_sign"]


@pytest.fixture(scope="module")
def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("P,N,short", [(P, N, s) for P, N in SHAPES for s in (False, True) if not (s and P == 1)])
@pytest.mark.parametrize("D", DIMS)
def test_records_equal_the_definition(lib, D, P, N, short):
    """Keys, reduced rows and int32 counts equal the fp64 definition exactly; the loss to 1e-5 relative.  n_pos = 2 P + 3 leaves a
    short last chunk, n_pos < P one short chunk (a chunk of one positive has no shorter form); the arrays are longer than n_pos (stride)."""
    import torch
    n_pos = P - 1 if short else 2 * P + 3
    ent_h, rel_h = lattice_tables(D, 17 * D + P)
    h, t, r, cand, pair, has = make_lists(P, N, n_pos, 1000 * D + 10 * P + N + int(short))
    if not short:
        for name in ("own_head", "masked_positive", "masked_chunk") + (("repeat", "out_of_range") if N >= 2 else ()) + (("other_positive",) if P >= 2 and N >= 3 else ()):
            assert name in has, name
    denom = n_pos * N
    want = ref.forward(ent_h, rel_h, h, t, r, cand, pair, P, MARGIN, denom)
    check_conditions(want)
    desc = desc_for(D, MARGIN)
    ent = torch.from_numpy(ent_h).cuda(); rel = torch.from_numpy(rel_h).cuda()
    rec, dst, loss = run_shared(lib, desc, ent, rel, h, t, r, cand, pair, P, n_pos + 5, denom)
    print("D %d P %d N %d n_pos %d: active %d of %d pairs, loss %.6f (fp64 %.6f), min kink %.2e, min sign %.2e"
          % (D, P, N, n_pos, int(want["active"].sum()), n_pos * N, loss, want["loss"], want["min_kink"], want["min_sign"]))
    assert np.array_equal(dst.cpu().numpy().astype(np.int64), want["keys"])
    if "masked_chunk" in has:
        j = has["masked_chunk"]
        assert (want["keys"][3 * n_pos + j * N:3 * n_pos + (j + 1) * N] == -1).all()
    rows, counts = reduce_on_device(lib, desc, rec, dst, D)
    want_rows, want_counts = ref.reduce(want["keys"], want["records"])
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(counts, want_counts)
    assert abs(loss - want["loss"]) <= 1e-5 * abs(want["loss"])


@pytest.mark.parametrize("D,P,N", [(50, 2, 63), (200, 64, 25)])
def test_no_active_pair_means_no_record(lib, D, P, N):
    """A margin so small that every hinge is off: every key is -1, the loss is zero, nothing is reduced."""
    import torch
    n_pos = 2 * P + 3
    ent_h, rel_h = lattice_tables(D, 5)
    h, t, r, cand, pair, _ = make_lists(P, N, n_pos, 77)
    want = ref.forward(ent_h, rel_h, h, t, r, cand, pair, P, -1000.0, n_pos * N)
    check_conditions(want)
    assert not want["active"].any()
    desc = desc_for(D, -1000.0)
    rec, dst, loss = run_shared(lib, desc, torch.from_numpy(ent_h).cuda(), torch.from_numpy(rel_h).cuda(), h, t, r, cand, pair, P, n_pos,
                                n_pos * N)
    assert (dst.cpu().numpy() == -1).all() and loss == 0.0
    rows, _ = reduce_on_device(lib, desc, rec, dst, D)
    assert len(rows) == 0


@pytest.mark.parametrize("P,N", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_equals_the_existing_emit_on_the_expanded_batch(lib, D, P, N):
    """Nothing masked: the lists spelled out as an ordinary batch -- negative k of positive b is (h_b, c_k, r_b) or
    (c_k, t_b, r_b) -- go through kge_transe_emit_records and the same reduce.  Rows and counts must be equal.  (Rows whose summed
    counts are all zero are dropped on both sides: the existing kernel keys the three slots of a positive by "some hinge is
    active", the shared kernel by "the slot's vector is not zero", and the two differ exactly on such rows.)"""
    import torch
    n_pos = 2 * P + 3
    stride = n_pos + 2
    ent_h, rel_h = lattice_tables(D, 31 * D + N)
    h, t, r, cand, pair, _ = make_lists(P, N, n_pos, 500 * D + P, mask=False)
    denom = n_pos * N
    want = ref.forward(ent_h, rel_h, h, t, r, cand, pair, P, MARGIN, denom)
    check_conditions(want)
    desc = desc_for(D, MARGIN)
    ent = torch.from_numpy(ent_h).cuda(); rel = torch.from_numpy(rel_h).cuda()
    rec, dst, loss = run_shared(lib, desc, ent, rel, h, t, r, cand, pair, P, stride, denom)
    rows, counts = reduce_on_device(lib, desc, rec, dst, D)
    bh, bt, br = ref.expand(h, t, r, cand, pair, P, stride)
    ids = [torch.from_numpy(x).cuda() for x in (bh, bt, br)]
    M = n_pos * (3 + N)
    dw = int(lib.kge_transe_record_dwords(ctypes.byref(desc)))
    rec2 = torch.zeros((M, dw), dtype=torch.int32, device="cuda")
    dst2 = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    loss2 = torch.zeros(1, dtype=torch.float32, device="cuda")
    lib.kge_set_option(b"tables_changed", 0)
    assert lib.kge_transe_emit_records(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), ids[0].data_ptr(), ids[1].data_ptr(),
                                       ids[2].data_ptr(), n_pos, N, stride, denom, rec2.data_ptr(), dst2.data_ptr(), None, None,
                                       loss2.data_ptr(), None) == 0
    nd = ctypes.c_int32(-1)
    assert lib.kge_transe_deferred_groups(ctypes.byref(nd)) == 0 and nd.value == 0
    rows2, counts2 = reduce_on_device(lib, desc, rec2, dst2, D)
    keep, keep2 = np.abs(counts).sum(1) > 0, np.abs(counts2).sum(1) > 0
    assert np.array_equal(rows[keep], rows2[keep2])
    assert np.array_equal(counts[keep], counts2[keep2])
    assert abs(loss - float(loss2.item())) <= 1e-5 * abs(loss)


def test_refusals(lib):
    """Every unsupported combination returns KGE_ERR_UNSUPPORTED with a message that names the limit."""
    import torch
    from openkeonspark_amd import _lib
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    f = torch.zeros((E + R, 1024), dtype=torch.float32, device="cuda")

    def call(desc, P, N):
        return lib.kge_transe_emit_records_shared(ctypes.byref(desc), f.data_ptr(), f.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                                  1, 1, P, z.data_ptr(), N, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), f.data_ptr(), None)

    for change, P, N, word in ((dict(model=1), 2, 2, "TransE"), (dict(negative_rel=1), 2, 2, "negative_rel"), ({}, 128, 2, "127"),
                               ({}, 2, 64, "63"), (dict(ent_dim=516, rel_dim=516), 2, 2, "512")):
        d = desc_for(8, 1.0)
        for k, v in change.items():
            setattr(d, k, v)
        assert call(d, P, N) == -4
        assert word in _lib.last_error(lib)
