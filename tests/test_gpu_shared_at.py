"""The two shared-negatives kernels on a SLICE of the batch (kge_shared_negatives_draw_at, kge_transe_emit_records_shared_at;
include/kge_mi355.h): chunk membership is a property of the global batch position, so the pieces of a batch cut anywhere must
add up to the one call over the whole batch -- the drawn lists row for row, the int8 records summed per destination key as
integers, the set of keyed rows, the loss to fp32 summation order.  One process, the C ABI.

The emit inputs are the lattice tables and hand-made lists of tests/test_gpu_shared_emit.py (no hinge decision and no sign within
rounding of its kink: asserted in fp64 by tests/shared_neg_ref.py before the device is looked at).  Every output sits between
sentinel margins."""
import ctypes

import numpy as np
import pytest

import shared_neg_ref as ref
from openkeonspark_amd import parallel
from openkeonspark_amd.train_paths import shared_chunk_span
from test_gpu_shared_draw import import_graph, make_graph
from test_gpu_shared_emit import E, MARGIN, check_conditions, desc_for, lattice_tables, make_lists

pytestmark = pytest.mark.gpu

PAD = 256             # sentinel bytes on both sides of every output
SENT = 0xA5


class Guarded:
    """`shape` elements of `dtype` in the middle of a byte allocation filled with SENT."""

    def __init__(self, shape, dtype):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.whole = torch.full((self.nbytes + 2 * PAD,), SENT, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.whole.data_ptr() + PAD

    def raw(self):
        """The middle's bytes; raises if a margin was written."""
        import torch
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        assert (w[:PAD] == SENT).all(), "written in front of the output"
        assert (w[PAD + self.nbytes:] == SENT).all(), "written behind the output"
        return w[PAD:PAD + self.nbytes].copy()

    def get(self):
        return self.raw().view(self.dtype).reshape(self.shape)


def slices_of_three_ranks(n_total):
    """The batch positions of 3 ranks sharing 8 sampler threads: [(first, n_pos)]."""
    return [parallel.slice_positions(n_total, 8, *parallel.thread_range(g, 3, 8)) for g in range(3)]


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    L.setBern(0)


# ---- draw --------------------------------------------------------------------------------------------------------------------
def draw(L, entry, h, t, r, first, P, N, seed, step):
    import torch
    from openkeonspark_amd import _lib
    n_pos = len(h)
    n_chunks = shared_chunk_span(max(first, 0), n_pos, max(P, 1))[1]      # (the refused calls get buffers all the same)
    ids = [torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.int32), np.zeros(1, np.int32)])).cuda() for x in (h, t, r)]
    cand, pair = Guarded((n_chunks, N), np.int32), Guarded((n_pos, N), np.uint8)
    _lib.check(getattr(L, entry)(ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n_pos, first, P, N, seed, step, cand.ptr(),
                                 pair.ptr(), None), L)
    return cand, pair


@pytest.mark.parametrize("P,N,n_total", [(4, 3, 23), (127, 2, 300), (1, 1, 7)])
def test_draw_of_a_piece_is_the_whole_batch_draw(lib, P, N, n_total):
    Eg = 7
    R, th, tt, tr = make_graph(Eg, 9)
    import_graph(lib, Eg, R, th, tt, tr, 1)
    pick = np.random.default_rng(P + N).integers(0, len(th), n_total)
    h, t, r = th[pick], tt[pick], tr[pick]
    seed, step = 0x1234ABCD5678EF01, 41
    cand, pair = (g.get() for g in draw(lib, "kge_shared_negatives_draw", h, t, r, 0, P, N, seed, step))
    if n_total >= 23:      # the lists are not degenerate: masked and unmasked pairs, both sides
        assert (pair & 2).any() and not (pair & 2).all() and {0, 1} <= set(np.unique(pair & 1))
    cuts = [slices_of_three_ranks(n_total)]
    if (P, N, n_total) == (4, 3, 23):
        cuts += [[(0, c), (c, n_total - c)] for c in range(1, n_total)]
    for pieces in cuts:
        assert sum(n for _, n in pieces) == n_total
        for first, n_pos in pieces:
            c0, n_chunks = shared_chunk_span(first, n_pos, P)
            gc, gp = draw(lib, "kge_shared_negatives_draw_at", h[first:first + n_pos], t[first:first + n_pos], r[first:first + n_pos],
                          first, P, N, seed, step)
            assert np.array_equal(gc.get(), cand[c0:c0 + n_chunks]), (first, n_pos)
            assert np.array_equal(gp.get(), pair[first:first + n_pos]), (first, n_pos)


def test_draw_at_refuses_what_draw_refuses_and_takes_an_empty_piece(lib):
    from openkeonspark_amd import _lib
    Eg = 7
    R, th, tt, tr = make_graph(Eg, 4)
    import_graph(lib, Eg, R, th, tt, tr, 0)
    for P_, N_, first, word in ((128, 2, 0, "127"), (2, 64, 0, "63"), (4, 2, -1, "bad arguments")):
        with pytest.raises(_lib.KgeError, match=word):
            draw(lib, "kge_shared_negatives_draw_at", th[:4], tt[:4], tr[:4], first, P_, N_, 0, 0)
    with pytest.raises(_lib.KgeError, match="multiple"):       # the older entry point keeps its rule
        draw(lib, "kge_shared_negatives_draw", th[:4], tt[:4], tr[:4], 3, 4, 2, 0, 0)
    cand, pair = draw(lib, "kge_shared_negatives_draw_at", th[:4], tt[:4], tr[:4], 3, 4, 2, 0, 0)      # ... which the new one lifts
    assert cand.get().shape == (2, 2) and pair.get().shape == (4, 2)
    cand, pair = draw(lib, "kge_shared_negatives_draw_at", th[:0], tt[:0], tr[:0], 5, 4, 2, 0, 0)
    assert cand.raw().size == 0 and pair.raw().size == 0       # (and the margins are whole)


# ---- emit --------------------------------------------------------------------------------------------------------------------
def emit(L, desc, ent, rel, h, t, r, cand, pair, first, P, denom, entry="kge_transe_emit_records_shared_at"):
    """One call over the positives h / t / r (global positions first ..) and their rows of the lists -> (records as int8
    [M, 4 dw], keys [M], loss, guarded buffers)."""
    import torch
    n_pos, N = pair.shape
    n_chunks = cand.shape[0]
    assert n_chunks == shared_chunk_span(first, n_pos, P)[1]
    M = 3 * n_pos + n_chunks * N
    dw = int(L.kge_transe_record_dwords(ctypes.byref(desc)))
    stride = n_pos + 3
    dev = lambda a: torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.int32), np.full(stride - len(a), 1 << 30, np.int32)])).cuda()
    dh, dt, dr = dev(h), dev(t), dev(r)
    dc = torch.from_numpy(np.ascontiguousarray(cand)).cuda() if cand.size else torch.zeros(1, dtype=torch.int32, device="cuda")
    dp = torch.from_numpy(np.ascontiguousarray(pair)).cuda() if pair.size else torch.zeros(1, dtype=torch.uint8, device="cuda")
    rec, dst, loss = Guarded((M, 4 * dw), np.int8), Guarded((M,), np.int32), Guarded((1,), np.float32)
    args = (ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), dh.data_ptr(), dt.data_ptr(), dr.data_ptr(), n_pos, stride)
    tail = (P, dc.data_ptr(), N, dp.data_ptr(), denom, rec.ptr(), dst.ptr(), loss.ptr(), None)
    fn = getattr(L, entry)
    rc = fn(*args, first, *tail) if entry.endswith("_at") else fn(*args, *tail)
    assert rc == 0
    return rec, dst, loss


def summed(keys, recs):
    """{key: int32 sum of its records' fields} over the keyed records."""
    out = {}
    for k, v in zip(keys, recs.astype(np.int32)):
        if k >= 0:
            out[int(k)] = out.get(int(k), 0) + v
    return out


@pytest.mark.parametrize("P,N", [(4, 3), (2, 63), (127, 2)])
@pytest.mark.parametrize("D", [4, 50, 200, 260, 512])
def test_pieces_add_up_to_the_whole_batch_call(lib, D, P, N):
    """The batch cut at the slice bounds of 3 ranks, and at an odd pair of bounds (a first piece of one position, a second that ends
    two positions into a chunk): records summed per key, the keyed rows and the loss against the one call."""
    import torch
    n_total = 2 * P + 3
    ent_h, rel_h = lattice_tables(D, 17 * D + P)
    h, t, r, cand, pair, _ = make_lists(P, N, n_total, 1000 * D + 10 * P + N)
    denom = n_total * N
    check_conditions(ref.forward(ent_h, rel_h, h, t, r, cand, pair, P, MARGIN, denom))
    desc = desc_for(D, MARGIN)
    ent, rel = torch.from_numpy(ent_h).cuda(), torch.from_numpy(rel_h).cuda()
    rec, dst, loss = emit(lib, desc, ent, rel, h, t, r, cand, pair, 0, P, denom)
    want, want_loss = summed(dst.get(), rec.get()), float(loss.get()[0])
    assert want and want_loss > 0
    odd = [(0, 1), (1, P + 1), (P + 2, n_total - P - 2)]
    for pieces in (slices_of_three_ranks(n_total), odd):
        assert sum(n for _, n in pieces) == n_total and any(f % P for f, _ in pieces)
        got, got_loss = {}, 0.0
        for first, n_pos in pieces:
            c0, n_chunks = shared_chunk_span(first, n_pos, P)
            sl = slice(first, first + n_pos)
            rec, dst, loss = emit(lib, desc, ent, rel, h[sl], t[sl], r[sl], cand[c0:c0 + n_chunks], pair[sl], first, P, denom)
            fields, keys = rec.get(), dst.get()
            assert np.abs(fields[:3 * n_pos].astype(np.int32)).max(initial=0) <= 2 * N
            assert np.abs(fields[3 * n_pos:].astype(np.int32)).max(initial=0) <= min(P, n_pos)
            for k, v in summed(keys, fields).items():
                got[k] = got.get(k, 0) + v
            got_loss += float(loss.get()[0])
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        print("D %d P %d N %d: %d keyed rows, loss %.7f in pieces, %.7f whole" % (D, P, N, len(want), got_loss, want_loss))
        assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss)


@pytest.mark.parametrize("D,P,N", [(50, 4, 3), (200, 2, 63), (512, 127, 2)])
def test_on_a_chunk_boundary_it_is_the_older_entry_point(lib, D, P, N):
    import torch
    n_pos = 2 * P + 3
    ent_h, rel_h = lattice_tables(D, 3 * D + N)
    h, t, r, cand, pair, _ = make_lists(P, N, n_pos, 7 * D + P)
    desc = desc_for(D, MARGIN)
    ent, rel = torch.from_numpy(ent_h).cuda(), torch.from_numpy(rel_h).cuda()
    old = emit(lib, desc, ent, rel, h, t, r, cand, pair, 0, P, n_pos * N, entry="kge_transe_emit_records_shared")
    for first in (0, 3 * P):
        new = emit(lib, desc, ent, rel, h, t, r, cand, pair, first, P, n_pos * N)
        for a, b in zip(old, new):
            assert np.array_equal(a.raw(), b.raw())


def test_emit_at_refuses_what_emit_refuses_and_takes_an_empty_piece(lib):
    import torch
    from openkeonspark_amd import _lib
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    f = torch.zeros((E + 5, 1024), dtype=torch.float32, device="cuda")

    def call(desc, P, N, first=1, n_pos=1):
        return lib.kge_transe_emit_records_shared_at(ctypes.byref(desc), f.data_ptr(), f.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                                     n_pos, 1, first, P, z.data_ptr(), N, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(),
                                                     f.data_ptr(), None)

    for change, P, N, word in ((dict(model=1), 2, 2, "TransE"), (dict(negative_rel=1), 2, 2, "negative_rel"), ({}, 128, 2, "127"),
                               ({}, 2, 64, "63"), (dict(ent_dim=516, rel_dim=516), 2, 2, "512")):
        d = desc_for(8, 1.0)
        for k, v in change.items():
            setattr(d, k, v)
        assert call(d, P, N) == -4
        assert word in _lib.last_error(lib)
    assert call(desc_for(8, 1.0), 2, 2, first=-1) == -3 and "bad arguments" in _lib.last_error(lib)
    assert call(desc_for(8, 1.0), 2, 2, n_pos=2) == -3          # stride < n_pos
    # no position: a zero loss, no record, no key
    ent_h, rel_h = lattice_tables(8, 1)
    none = np.zeros(0, np.int32)
    rec, dst, loss = emit(lib, desc_for(8, MARGIN), torch.from_numpy(ent_h).cuda(), torch.from_numpy(rel_h).cuda(), none, none, none,
                          np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8), 5, 4, 12)
    assert rec.raw().size == 0 and dst.raw().size == 0 and float(loss.get()[0]) == 0.0
