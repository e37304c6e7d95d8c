"""The six TransE emit entry points on the exact tables of tests/dyadic_cases.py: kge_transe_emit_records,
kge_transe_emit_records_bf16, kge_transe_emit_records_shared, _shared_chunks, _shared_bf16 and _shared_chunks_bf16.

On those tables every intermediate value of the definition is a float32 value (premises, asserted on the CPU before the device
is looked at), so the fp64 references are the truth bit for bit and NOTHING is excused: no tolerance, no radius around a kink, no
element left out.  Hundreds of hinges are exactly zero (a tie is active) or one quantum either side of it; more than half of the
elements of e are exact zeros, from all-zero operands, from cancellation and from -0.0 operands (sign(+-0) = 0); the all +0.0,
all -0.0 and clipped rows are head, tail, relation, corrupted entity and candidate.

  keys                    equal the reference
  records                 every one of the D element bytes of every live record (the first D bytes; see `elements`)
  loss                    the bits of np.float32(reference loss): every partial sum is exact, whatever its order
  deferred groups         kge_transe_deferred_groups
  kge_transe_reduce_records on the device's records gives the reference's per-row counts
  bf16 kernels            equal the fp32 kernels on the widened tables word for word

From 63 negatives on, group X_POS has exactly 63 active negatives, all new tails whose sign opposes the positive's in one column:
its head record holds +-126 there, the largest sum an int8 record can get.  At 70 negatives (bf16 only: the fp32 entry point
takes at most 63) group Y_POS has exactly 64: deferred -- keys -1, counted, not in the loss."""
import ctypes

import numpy as np
import pytest

import bf16_ref
import dyadic_cases as dc
from test_gpu_bf16_shared_emit import on_device, run_bf16
from test_gpu_shared_emit import reduce_on_device, run_shared
from test_gpu_shared_emit_chunks import run_chunks

pytestmark = pytest.mark.gpu

TRANSE = 0


@pytest.fixture(scope="module")
def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


def desc_for(D, margin):
    from openkeonspark_amd import _lib
    return _lib.ModelDesc(TRANSE, 0, dc.E, dc.R, D, D, margin, 0)


def bits(x):
    return int(np.float32(x).view(np.uint32))


def elements(rec, D):
    """int8 records [M, bytes] -> the D elements of each.  A width that is a multiple of 4 has byte e = element e.  Any other
    width takes the plain rung (L, C) of csrc/team_shape.hpp and the strided layout kge_transe_reduce_records reads for it: lane l
    of the team holds elements l, l + L, ..., its c-th one in byte c % 4 of dword l + L (c / 4)."""
    if D % 4 == 0:
        return rec[:, :D]
    L = 16 if D <= 64 else 32 if D <= 128 else 64
    e = np.arange(D)
    lane, c = e % L, e // L
    return rec[:, 4 * (lane + L * (c // 4)) + c % 4]


def run_batch(L, c, bf16):
    """-> (keys, records as int8 [M, 4 dw], loss bits, deferred groups, the device tensors of records and keys)."""
    import torch
    from openkeonspark_amd import _lib
    D, n_neg = c["D"], c["n_neg"]
    desc = desc_for(D, c["margin"])
    dw = int(L.kge_transe_record_dwords(ctypes.byref(desc)))
    M = dc.N_POS * (3 + n_neg)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bh, bt, br = d(c["bh"]), d(c["bt"]), d(c["br"])
    rec = torch.full((M, dw), 0x55555555, dtype=torch.int32, device="cuda")
    dst = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    if bf16:
        ent, rel = on_device(bf16_ref.to_bf16(c["ent"])), on_device(bf16_ref.to_bf16(c["rel"]))
        _lib.check(L.kge_transe_emit_records_bf16(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), bh.data_ptr(), bt.data_ptr(), br.data_ptr(),
                                                  dc.N_POS, n_neg, dc.STRIDE, dc.DENOM, rec.data_ptr(), dst.data_ptr(), loss.data_ptr(), None), L)
    else:
        ent, rel = d(c["ent"]), d(c["rel"])
        L.kge_set_option(b"tables_changed", 1)      # fresh tensors may reuse an address whose 1/|row| table the engine still holds
        _lib.check(L.kge_transe_emit_records(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), bh.data_ptr(), bt.data_ptr(), br.data_ptr(),
                                             dc.N_POS, n_neg, dc.STRIDE, dc.DENOM, rec.data_ptr(), dst.data_ptr(), None, None, loss.data_ptr(),
                                             None), L)
    nd = ctypes.c_int32(-1)
    _lib.check(L.kge_transe_deferred_groups(ctypes.byref(nd)), L)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), rec.cpu().numpy().view(np.int8).reshape(M, 4 * dw), bits(loss.item()), nd.value, rec, dst


def check_batch(L, c, got):
    keys, rec, loss_bits, deferred, d_rec, d_dst = got
    want, D, n_neg = c["want"], c["D"], c["n_neg"]
    assert deferred == want["deferred"]
    np.testing.assert_array_equal(keys, want["keys"])
    live = want["keys"] >= 0
    assert live.sum() > dc.N_POS
    np.testing.assert_array_equal(elements(rec[live], D), want["rec"][live])
    print("loss %.9g reference %.9g" % (np.uint32(loss_bits).view(np.float32), want["loss"]))
    assert loss_bits == bits(want["loss"])
    rows, counts = reduce_on_device(L, desc_for(D, c["margin"]), d_rec, d_dst, D)
    order = np.argsort(rows)
    want_rows, want_counts = bf16_ref.row_counts(want["keys"], want["rec"])
    np.testing.assert_array_equal(rows[order], want_rows)
    np.testing.assert_array_equal(counts[order], want_counts)
    by_group = keys.reshape(3 + n_neg, dc.N_POS)
    if n_neg >= 63:                                          # 63 active negatives: recorded, and a byte of the head record is +-126
        assert (by_group[:3, dc.X_POS] >= 0).all() and (by_group[3:66, dc.X_POS] >= 0).all() and (by_group[66:, dc.X_POS] == -1).all()
        assert np.abs(elements(rec, D).reshape(3 + n_neg, dc.N_POS, D)[0, dc.X_POS].astype(np.int32)).max() == 126
    if n_neg >= 64:                                          # 64: deferred
        assert (by_group[:, dc.Y_POS] == -1).all() and deferred >= 1


@pytest.mark.parametrize("n_neg", dc.NEGS)
@pytest.mark.parametrize("D", dc.FP32_DIMS)
def test_emit_records(lib, D, n_neg):
    c = dc.batch_case(D, n_neg)
    check_batch(lib, c, run_batch(lib, c, bf16=False))


@pytest.mark.parametrize("n_neg", dc.NEGS + [dc.BOUNDARY_NEG])
@pytest.mark.parametrize("D", dc.BF16_DIMS)
def test_emit_records_bf16(lib, D, n_neg):
    c = dc.batch_case(D, n_neg)
    got = run_batch(lib, c, bf16=True)
    check_batch(lib, c, got)
    if n_neg <= 63:                                          # the fp32 kernel on the widened tables, word for word
        keys32, rec32, loss32, deferred32, _, _ = run_batch(lib, c, bf16=False)
        np.testing.assert_array_equal(got[0], keys32)
        live = keys32 >= 0
        np.testing.assert_array_equal(got[1][live][:, :D], rec32[live][:, :D])
        assert got[2] == loss32 and got[3] == deferred32


def check_lists(L, c, rec, dst, loss):
    want, D = c["want"], c["D"]
    keys = dst.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(keys, want["keys"])
    live = keys >= 0
    assert live.sum() > 3
    got = elements(rec.cpu().numpy().view(np.int8).reshape(len(keys), -1), D).astype(np.int64)
    np.testing.assert_array_equal(got[live], want["records"][live])
    print("loss %.9g reference %.9g" % (float(loss.item()), want["loss"]))
    assert bits(loss.item()) == bits(want["loss"])
    rows, counts = reduce_on_device(L, desc_for(D, c["margin"]), rec, dst, D)
    order = np.argsort(rows)
    want_rows, want_counts = bf16_ref.row_counts(want["keys"], want["records"])
    np.testing.assert_array_equal(rows[order], want_rows)
    np.testing.assert_array_equal(counts[order], want_counts)
    b = c["masked_positive"]
    assert (keys[[b, c["n_pos"] + b, 2 * c["n_pos"] + b]] == -1).all()


def run_lists(L, c, bf16):
    import torch
    desc = desc_for(c["D"], c["margin"])
    stride = c["n_pos"] + 5
    args = (c["h"], c["t"], c["r"], c["cand"], c["pair"])
    if bf16:
        ent, rel = on_device(bf16_ref.to_bf16(c["ent"])), on_device(bf16_ref.to_bf16(c["rel"]))
        rec, dst, loss = run_bf16(L, desc, ent, rel, *args, c["P"], None if c["by_position"] else c["table"], stride, dc.DENOM)
    else:
        ent, rel = torch.from_numpy(c["ent"]).cuda(), torch.from_numpy(c["rel"]).cuda()
        L.kge_set_option(b"tables_changed", 1)
        if c["by_position"]:
            rec, dst, loss = run_shared(L, desc, ent, rel, *args, c["P"], stride, dc.DENOM)
            loss = torch.tensor([loss], dtype=torch.float32)
        else:
            rec, dst, loss = run_chunks(L, desc, ent, rel, *args, c["table"], stride, dc.DENOM)
    return rec.contiguous(), dst.contiguous(), loss


@pytest.mark.parametrize("P,N", dc.SHARED_SHAPES)
@pytest.mark.parametrize("D", dc.FP32_DIMS)
def test_emit_records_shared(lib, D, P, N):
    c = dc.lists_case(D, P, N)
    check_lists(lib, c, *run_lists(lib, c, bf16=False))


@pytest.mark.parametrize("P,N", dc.SHARED_SHAPES)
@pytest.mark.parametrize("D", dc.FP32_DIMS)
def test_emit_records_shared_chunks(lib, D, P, N):
    c = dc.chunks_case(D, P, N)
    rec, dst, loss = run_lists(lib, c, bf16=False)
    check_lists(lib, c, rec, dst, loss)
    assert (dst.cpu().numpy()[3 * c["n_pos"] + (len(c["table"]) - 2) * N:] == -1).all()      # the empty slots' candidate keys


@pytest.mark.parametrize("by_position", [True, False])
@pytest.mark.parametrize("P,N", dc.SHARED_SHAPES)
@pytest.mark.parametrize("D", dc.SHARED_BF16_DIMS)
def test_emit_records_shared_bf16(lib, D, P, N, by_position):
    import torch
    c = dc.lists_case(D, P, N) if by_position else dc.chunks_case(D, P, N)
    rec, dst, loss = run_lists(lib, c, bf16=True)
    check_lists(lib, c, rec, dst, loss)
    rec32, dst32, loss32 = run_lists(lib, c, bf16=False)     # the fp32 kernel on the widened tables, word for word
    assert torch.equal(dst, dst32) and torch.equal(rec, rec32)
    assert bits(loss.item()) == bits(loss32.item())
