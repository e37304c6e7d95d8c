"""kge_transe_emit_records_shared_bf16 / kge_transe_emit_records_shared_chunks_bf16 alone (include/kge_mi355.h, "Shared negatives on
bf16 tables"), on the lattice tables of tests/test_gpu_shared_emit.py rounded to bf16 and that module's hand-made lists.

Before the device is looked at, the fp64 definition (tests/shared_neg_ref.py) on the WIDENED tables must meet that module's
  kink condition  no unmasked pair with |p - n + margin| < 1e-4
  sign condition  no element |h^ + r^ - t^| < 1e-5 in any scored triple
(rounding the lattice to bf16 moves 0.1, 0.3 and 0.07 by less than half a percent: still three magnitudes whose signed sums stay
about 0.1 / sqrt(D) from zero).  Then, with nothing excused:
  1. keys and the first D bytes of every live record equal the fp64 definition;
  2. keys, every record word and the float32 loss are bit-identical to kge_transe_emit_records_shared on the widened tables --
     no tolerance: after the widening the two kernels are the same code;
  3. the same two for the `_chunks` entry point on a table from train_paths.shared_relation_chunks, with empty slots and relation
     runs shorter than P;
  4. kge_transe_reduce_records on the records gives the definition's per-row counts.
Widths 8 .. 512 sit on both sides of the kernel's one / two elements-of-four per lane (256 | 264) and of the tile split
(N = 63 and 25 at width 512 take more than one LDS tile); n_pos = 2 P + 3 leaves a short last chunk."""
import ctypes

import numpy as np
import pytest

import bf16_ref
import shared_neg_ref as ref
from test_gpu_shared_emit import E, MARGIN, R, check_conditions, desc_for, lattice_tables, make_lists, reduce_on_device, run_shared
from test_gpu_shared_emit_chunks import forward_chunks, run_chunks
from test_gpu_shared_emit_chunks import make_lists as make_chunk_lists

pytestmark = pytest.mark.gpu

DIMS = [8, 64, 200, 256, 264, 512]
SHAPES = [(1, 1), (2, 63), (64, 25), (127, 2)]


@pytest.fixture(scope="module")
def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


def bf16_tables(D, seed):
    """(ent bits, rel bits, ent widened, rel widened): the lattice rounded to bf16 and its exact fp32 widening."""
    ent, rel = lattice_tables(D, seed)
    eb, rb = bf16_ref.to_bf16(ent), bf16_ref.to_bf16(rel)
    return eb, rb, bf16_ref.widen(eb), bf16_ref.widen(rb)


def on_device(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()


def run_bf16(L, desc, ent, rel, h, t, r, cand, pair, P, chunks, stride, denom):
    """The bf16 entry point (chunks None: by position) on buffers prefilled like run_shared's / run_chunks' -> rec, dst, loss tensors."""
    import torch
    n_pos, N = pair.shape
    slots = cand.shape[0] if chunks is None else len(chunks)
    M = 3 * n_pos + slots * N
    dw = int(L.kge_transe_record_dwords(ctypes.byref(desc)))
    dev = lambda a, n: torch.from_numpy(np.concatenate([a, np.zeros(n - len(a), a.dtype)])).cuda()
    dh, dt, dr = dev(h, stride), dev(t, stride), dev(r, stride)
    dc, dp = torch.from_numpy(cand).cuda(), torch.from_numpy(pair).cuda()
    rec = torch.full((M + 1, dw), 0x55, dtype=torch.int32, device="cuda")
    dst = torch.full((M + 1,), -7, dtype=torch.int32, device="cuda")
    loss = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    if chunks is None:
        rc = L.kge_transe_emit_records_shared_bf16(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), dh.data_ptr(), dt.data_ptr(), dr.data_ptr(),
                                                   n_pos, stride, P, dc.data_ptr(), N, dp.data_ptr(), denom, rec.data_ptr(), dst.data_ptr(),
                                                   loss.data_ptr(), None)
    else:
        dtab = torch.from_numpy(np.ascontiguousarray(chunks)).cuda()
        rc = L.kge_transe_emit_records_shared_chunks_bf16(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), dh.data_ptr(), dt.data_ptr(),
                                                          dr.data_ptr(), n_pos, stride, dtab.data_ptr(), len(chunks), dc.data_ptr(), N,
                                                          dp.data_ptr(), denom, rec.data_ptr(), dst.data_ptr(), loss.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(dst[M].item()) == -7 and (rec[M] == 0x55).all()      # nothing past the last record
    return rec[:M].contiguous(), dst[:M].contiguous(), loss


def check_against_definition(L, desc, D, rec, dst, loss, want):
    keys = dst.cpu().numpy().astype(np.int64)
    assert np.array_equal(keys, want["keys"])                                       # 1. keys ...
    live = keys >= 0
    assert live.any()
    got = rec.cpu().numpy().view(np.int8)[:, :D].astype(np.int64)
    assert np.abs(want["records"]).max() <= 127
    assert np.array_equal(got[live], want["records"][live])                         # ... and the first D bytes of every live record
    rows, counts = reduce_on_device(L, desc, rec, dst, D)                           # 4. the reduce serves unchanged
    want_rows, want_counts = ref.reduce(want["keys"], want["records"])
    assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts)
    assert abs(float(loss.item()) - want["loss"]) <= 1e-5 * abs(want["loss"])


def bits_of(loss):
    return int(np.float32(loss).view(np.uint32))


@pytest.mark.parametrize("P,N", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_chunks_by_position(lib, D, P, N):
    import torch
    assert lib.kge_bf16_shared_supported(ctypes.byref(desc_for(D, MARGIN)), N) == 1
    n_pos = 2 * P + 3
    eb, rb, ent_w, rel_w = bf16_tables(D, 17 * D + P)
    h, t, r, cand, pair, has = make_lists(P, N, n_pos, 1000 * D + 10 * P + N)
    assert "own_head" in has and "masked_positive" in has
    denom = n_pos * N
    want = ref.forward(ent_w, rel_w, h, t, r, cand, pair, P, MARGIN, denom)
    check_conditions(want)
    desc = desc_for(D, MARGIN)
    rec, dst, loss = run_bf16(lib, desc, on_device(eb), on_device(rb), h, t, r, cand, pair, P, None, n_pos + 5, denom)
    print("D %d P %d N %d n_pos %d: active %d of %d pairs, loss %.9g (fp64 %.9g), min kink %.2e, min sign %.2e"
          % (D, P, N, n_pos, int(want["active"].sum()), n_pos * N, float(loss.item()), want["loss"], want["min_kink"], want["min_sign"]))
    check_against_definition(lib, desc, D, rec, dst, loss, want)
    # 2. the fp32 kernel on the widened tables, bit for bit
    rec32, dst32, loss32 = run_shared(lib, desc, torch.from_numpy(ent_w).cuda(), torch.from_numpy(rel_w).cuda(), h, t, r, cand, pair, P,
                                      n_pos + 5, denom)
    assert torch.equal(dst, dst32) and torch.equal(rec, rec32)
    assert bits_of(loss.item()) == bits_of(loss32)


@pytest.mark.parametrize("P,N", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_chunks_from_the_relation_order(lib, D, P, N):
    import torch
    from openkeonspark_amd.train_paths import shared_chunk_cap, shared_relation_chunks
    n_pos = 2 * P + 3
    eb, rb, ent_w, rel_w = bf16_tables(D, 19 * D + P)
    seed = 2000 * D + 10 * P + N
    cap = shared_chunk_cap(n_pos, P, R)
    h, t, r, cand, pair = make_chunk_lists(n_pos, cap, N, seed)
    r[:(3 * n_pos) // 5] = 0                                                        # one run longer than P, the others shorter
    perm, chunks, n_chunks = shared_relation_chunks(r, P, R)
    h, t, r2 = h[perm], t[perm], r[perm]
    cand[0, 0] = h[0]; pair[0, 0] = 0                                               # (the first positive's own head as a new tail)
    assert len(chunks) == cap and n_chunks < cap and (chunks[n_chunks:, 1] == 0).all()      # empty slots
    assert (chunks[:n_chunks, 1] == P).any() and (P == 1 or (chunks[:n_chunks, 1] < P).any())      # full chunks, and runs shorter than P
    denom = n_pos * N
    want = forward_chunks(ent_w, rel_w, h, t, r2, cand, pair, chunks, MARGIN, denom)
    check_conditions(want)
    desc = desc_for(D, MARGIN)
    rec, dst, loss = run_bf16(lib, desc, on_device(eb), on_device(rb), h, t, r2, cand, pair, 0, chunks, n_pos + 5, denom)
    check_against_definition(lib, desc, D, rec, dst, loss, want)
    assert (dst.cpu().numpy()[3 * n_pos + n_chunks * N:] == -1).all()               # the empty slots' candidate keys
    rec32, dst32, loss32 = run_chunks(lib, desc, torch.from_numpy(ent_w).cuda(), torch.from_numpy(rel_w).cuda(), h, t, r2, cand, pair, chunks,
                                      n_pos + 5, denom)
    assert torch.equal(dst, dst32) and torch.equal(rec, rec32.contiguous())
    assert bits_of(loss.item()) == bits_of(loss32.item())


def test_refusals(lib):
    """Each with kge_bf16_shared_supported == 0, KGE_ERR_UNSUPPORTED from both entry points and the reason in the message."""
    import torch
    from openkeonspark_amd import _lib
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    f = torch.zeros((E + R, 1024), dtype=torch.int16, device="cuda")
    out = torch.zeros(4, dtype=torch.float32, device="cuda")
    table = torch.tensor([[0, 1]], dtype=torch.int32, device="cuda")
    p = z.data_ptr()

    def by_position(desc, N):
        return lib.kge_transe_emit_records_shared_bf16(ctypes.byref(desc), f.data_ptr(), f.data_ptr(), p, p, p, 1, 1, 2, p, N, p, 1, p, p,
                                                       out.data_ptr(), None)

    def by_table(desc, N):
        return lib.kge_transe_emit_records_shared_chunks_bf16(ctypes.byref(desc), f.data_ptr(), f.data_ptr(), p, p, p, 1, 1, table.data_ptr(), 1,
                                                              p, N, p, 1, p, p, out.data_ptr(), None)

    for change, N, word in ((dict(ent_dim=100, rel_dim=100), 2, "multiple of 8"), (dict(ent_dim=520, rel_dim=520), 2, "512"), ({}, 64, "63"),
                            (dict(negative_rel=1), 2, "negative_rel"), (dict(model=1), 2, "TransE")):
        d = desc_for(8, 1.0)
        for k, v in change.items():
            setattr(d, k, v)
        assert lib.kge_bf16_shared_supported(ctypes.byref(d), N) == 0
        for call in (by_position, by_table):
            assert call(d, N) == -4
            assert word in _lib.last_error(lib) and "bf16" in _lib.last_error(lib)
    for D, N in ((8, 1), (512, 63)):
        assert lib.kge_bf16_shared_supported(ctypes.byref(desc_for(D, 1.0)), N) == 1
    lib.kge_clear_error()
