"""The device stages of the table-sharded sparse TransE step (csrc/shard.hip, the record reduction and the row-list updates of
csrc/transe_counts.hip), each called through the C ABI as train_paths.sharded_step calls it and compared with a few lines of numpy
written from the header's description (include/kge_mi355.h, "Table-sharded sparse path").  Every stage is integer work or a
copy, so every comparison is exact.

Two habits throughout: every output is the middle of a larger allocation, itself and the margins on both sides filled with a
sentinel, and the margins plus every element the stage has no business writing must still hold the sentinel afterwards; and the
row gather reads its table as a view into an allocation with sentinel rows before and after, so that an id from outside the
shard shows a missing clamp as a wrong value (the documented result is table[clip(id - row_lo, 0, rows - 1)])."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = -1515870811          # 0xA5A5A5A5 as int32; as a float32 bit pattern -2.87e-16: no id, count, slot or table value used here
MARGIN = 64                 # int32 elements (256 bytes: the 16-byte accesses of the copy kernels stay aligned)
KGE_ERR_BAD_ARG = -3
DIMS = [4, 48, 64, 68, 128, 200, 256, 260, 512, 1024]     # every branch of transe_team_shape, both sides of the 64-dword line
RECORD_DWORDS = {4: 16, 48: 16, 64: 16, 68: 32, 128: 32, 200: 64, 256: 64, 260: 128, 512: 128, 1024: 256}
SCALAR_DIMS = [7, 30]     # the two scalar rungs (16, 1) and (16, 2), which only widths that are no multiple of 4 take
RECORD_DWORDS.update({7: 16, 30: 16})


def _env():
    import torch
    from openkeonspark_amd import _lib
    return torch, _lib, _lib.lib()


class Guarded:
    """`n` int32 elements (any shape) in the middle of an allocation of n + 2 * MARGIN, everything filled with SENT."""

    def __init__(self, *shape):
        import torch
        self.n = int(np.prod(shape)) if shape else 1
        self.whole = torch.full((self.n + 2 * MARGIN,), SENT, dtype=torch.int32, device="cuda")
        self.t = self.whole[MARGIN:MARGIN + self.n].view(*shape)

    def put(self, values):
        import torch
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).view(self.t.shape))
        return self

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        """The middle as numpy; raises if a margin was written."""
        import torch
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        assert (w[:MARGIN] == SENT).all(), "the stage wrote in front of its output"
        assert (w[MARGIN + self.n:] == SENT).all(), "the stage wrote behind its output"
        return w[MARGIN:MARGIN + self.n].reshape(tuple(self.t.shape)).copy()


def _dev(values, dtype=np.int32):
    """A device copy; the caller keeps the tensor for as long as a launch reads it."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype=dtype)).cuda()


def _desc(_lib, ent_total, rel_total, dim):
    return _lib.ModelDesc(_lib.TRANSE, 0, int(ent_total), int(rel_total), int(dim), int(dim), 1.0, 0)


def _ok(rc, _lib):
    assert rc == 0, _lib.last_error()


# ---- inputs ----------------------------------------------------------------------------------------------------------------

JUNK = 1 << 30      # what the unused tail [n_pos, stride) of every batch block holds: no stage may read it


def make_batch(rng, n_pos, n_ent_neg, n_rel_neg, stride, E, R):
    """(h, t, r), each [(1 + n_neg) * stride], in the sampler's layout (Base.cpp:109-139): the positives at [0, n_pos), negative k
    of positive b at b + (k + 1) * stride, entity-corrupted negatives first, then the relation-corrupted ones.  Every negative
    differs from its positive in exactly one slot (the new value drawn until it differs); about one positive in eight is a
    self-loop."""
    n_neg = n_ent_neg + n_rel_neg
    h = np.full((1 + n_neg, stride), JUNK, np.int64); t = h.copy(); r = h.copy()
    ph = rng.integers(0, E, n_pos); pt = rng.integers(0, E, n_pos); pr = rng.integers(0, R, n_pos)
    loop = rng.random(n_pos) < 0.125
    pt[loop] = ph[loop]
    h[0, :n_pos], t[0, :n_pos], r[0, :n_pos] = ph, pt, pr

    def other(old, total):
        new = rng.integers(0, total, n_pos)
        while (new == old).any():
            same = new == old
            new[same] = rng.integers(0, total, int(same.sum()))
        return new

    for k in range(n_neg):
        nh, nt, nr = ph.copy(), pt.copy(), pr.copy()
        if k < n_ent_neg:
            head = rng.random(n_pos) < 0.5
            nh[head] = other(ph, E)[head]
            nt[~head] = other(pt, E)[~head]
        else:
            nr = other(pr, R)
        assert (((nh != ph).astype(int) + (nt != pt) + (nr != pr)) == 1).all()
        h[k + 1, :n_pos], t[k + 1, :n_pos], r[k + 1, :n_pos] = nh, nt, nr
    return h.reshape(-1), t.reshape(-1), r.reshape(-1)


def requests_reference(h, t, n_pos, n_neg, stride):
    """req[slot * n_pos + b]: slot 0 / 1 = the positive's head / tail, 2 = its relation (no entity), 3 + k = the NEW entity of
    negative k, -1 if it has none (a relation-corrupted negative)."""
    req = np.full((3 + n_neg, n_pos), -1, np.int64)
    req[0], req[1] = h[:n_pos], t[:n_pos]
    for k in range(n_neg):
        nh, nt = h[(k + 1) * stride:][:n_pos], t[(k + 1) * stride:][:n_pos]
        req[3 + k] = np.where(nh != h[:n_pos], nh, np.where(nt != t[:n_pos], nt, -1))
    return req.reshape(-1)


def make_records(rng, n, dim):
    """[n, dwords] int32 records in the natural layout of widths that are multiples of 4: viewed as int8, byte e of a record is
    element e for e < dim (random in [-63, 63]), the pad bytes zero -- and the same values as an [n, dim] int8 matrix."""
    dw = RECORD_DWORDS[dim]
    vals = rng.integers(-63, 64, (n, dim)).astype(np.int8)
    rec = np.zeros((n, 4 * dw), np.int8)
    rec[:, :dim] = vals
    return rec.view(np.int32).reshape(n, dw), vals


def sums_by_row(vals, dst, keep):
    """(rows, sums): the sorted distinct destinations among dst[keep] and the int64 column sums of their records."""
    idx = np.nonzero(keep)[0]
    order = idx[np.argsort(dst[idx], kind="stable")]
    rows, first = np.unique(dst[order], return_index=True)
    if len(rows) == 0:
        return rows, np.zeros((0, vals.shape[1]), np.int64)
    return rows, np.add.reduceat(vals[order].astype(np.int64), first, axis=0)


# ---- the counting sort by owner -----------------------------------------------------------------------------------------------

def run_count(ids, chunk, owners):
    torch, _lib, L = _env()
    d_ids = _dev(ids)
    counts = Guarded(owners)
    _ok(L.kge_shard_count(d_ids.data_ptr(), len(ids), chunk, owners, counts.ptr(), None), _lib)
    return d_ids, counts.get()


def run_scatter(d_ids, n, chunk, owners, counts):
    torch, _lib, L = _env()
    cursor, srt, slot_of = Guarded(owners), Guarded(max(n, 1)), Guarded(max(n, 1))
    h_counts = (ctypes.c_int64 * owners)(*[int(c) for c in counts])
    _ok(L.kge_shard_scatter(d_ids.data_ptr(), n, chunk, owners, h_counts, cursor.ptr(), srt.ptr(), slot_of.ptr(), None), _lib)
    cursor.get()
    return srt.get()[:n], slot_of.get()[:n]


def check_count_and_scatter(ids, chunk, owners, what):
    """kge_shard_count against np.bincount, then kge_shard_scatter's contract (the order inside an owner's group is free)."""
    ids = np.asarray(ids, np.int64)
    n, live = len(ids), ids >= 0
    n_live = int(live.sum())
    d_ids, counts = run_count(ids, chunk, owners)
    want = np.bincount(ids[live] // chunk, minlength=owners)
    assert np.array_equal(counts, want), (what, counts, want)
    srt, slot_of = run_scatter(d_ids, n, chunk, owners, counts)
    assert np.array_equal(slot_of == -1, ~live), what
    assert np.array_equal(np.sort(slot_of[live]), np.arange(n_live)), what           # a permutation of range(n_live)
    assert np.array_equal(srt[slot_of[live]], ids[live]), what
    assert (srt[n_live:] == SENT).all(), what                                       # nothing behind the live ids
    own = srt[:n_live] // chunk
    assert (np.diff(own) >= 0).all(), what
    assert np.array_equal(np.bincount(own, minlength=owners), want), what
    return srt, slot_of


@pytest.mark.parametrize("owners", [1, 2, 3, 7, 64])
def test_count_and_scatter_by_owner(owners):
    """Id lists of 1, 2047, 2048, 2049 and 100 000 ids (one scatter workgroup takes 2048), a fifth of them -1, over 1 .. 64
    owners of an entity count the owners do not divide; the all -1 list; the list that falls to one owner."""
    from openkeonspark_amd import parallel
    rng = np.random.default_rng(100 + owners)
    E = 64 * 1563 + 37
    assert owners == 1 or E % owners
    chunk = parallel.chunk_size(E, owners)
    for n in (1, 2047, 2048, 2049, 100_000):
        ids = rng.integers(0, E, n)
        if n > 1:
            ids[rng.random(n) < 0.2] = -1
            ids[-1] = E - 1                      # the last row of the last (short) shard
        check_count_and_scatter(ids, chunk, owners, ("mixed", owners, n))
        check_count_and_scatter(np.full(n, -1), chunk, owners, ("all -1", owners, n))
        o = owners // 2
        lo, hi = o * chunk, min((o + 1) * chunk, E)
        check_count_and_scatter(rng.integers(lo, hi, n), chunk, owners, ("one owner", owners, n))


def test_count_and_scatter_at_config5_ids():
    """Ids as large as BASELINE config #5's: 50 000 000 entities over 8 owners."""
    from openkeonspark_amd import parallel
    rng = np.random.default_rng(5)
    E, W = 50_000_000, 8
    chunk = parallel.chunk_size(E, W)
    ids = rng.integers(0, E, 100_000)
    ids[rng.random(len(ids)) < 0.1] = -1
    ids[:4] = [E - 1, 0, chunk - 1, chunk]
    check_count_and_scatter(ids, chunk, W, "config 5")


def test_scatter_refuses_inconsistent_counts_and_too_many_owners():
    torch, _lib, L = _env()
    n = 100
    d_ids = _dev(np.arange(n))
    cursor, srt, slot_of, counts = Guarded(65), Guarded(n), Guarded(n), Guarded(65)
    too_many = (ctypes.c_int64 * 2)(60, 41)                 # 101 ids announced, 100 given
    assert L.kge_shard_scatter(d_ids.data_ptr(), n, 50, 2, too_many, cursor.ptr(), srt.ptr(), slot_of.ptr(), None) == KGE_ERR_BAD_ARG
    h65 = (ctypes.c_int64 * 65)(*([1] * 65))
    assert L.kge_shard_scatter(d_ids.data_ptr(), n, 2, 65, h65, cursor.ptr(), srt.ptr(), slot_of.ptr(), None) == KGE_ERR_BAD_ARG
    assert L.kge_shard_count(d_ids.data_ptr(), n, 2, 65, counts.ptr(), None) == KGE_ERR_BAD_ARG
    for g in (cursor, srt, slot_of, counts):                # a refused call writes nothing
        assert (g.get() == SENT).all()
    exact = (ctypes.c_int64 * 2)(50, 50)
    _ok(L.kge_shard_scatter(d_ids.data_ptr(), n, 50, 2, exact, cursor.ptr(), srt.ptr(), slot_of.ptr(), None), _lib)
    assert np.array_equal(np.sort(slot_of.get()), np.arange(n))


# ---- requests and the remapped batch ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_neg,n_rel_neg", [(1, 0), (3, 0), (3, 2), (25, 0), (25, 2)])
def test_requests_and_remapped_batch(n_neg, n_rel_neg):
    """kge_shard_requests element for element; then, on the counting sort of those requests, kge_shard_remap_batch: every triple
    of the batch finds its own head and tail behind the slots it was given, a kept side of a negative carries exactly its
    positive's slot, a relation-corrupted negative both."""
    torch, _lib, L = _env()
    from openkeonspark_amd import parallel
    rng = np.random.default_rng(1000 * n_neg + n_rel_neg)
    E, R, W = 1003, 11, 7
    chunk = parallel.chunk_size(E, W)
    for n_pos in (1, 255, 256, 257, 5000):
        for stride in (n_pos, n_pos + 37):
            what = (n_pos, n_neg, n_rel_neg, stride)
            h, t, r = make_batch(rng, n_pos, n_neg - n_rel_neg, n_rel_neg, stride, E, R)
            d_h, d_t, d_r = _dev(h), _dev(t), _dev(r)
            M = n_pos * (3 + n_neg)
            req = Guarded(M)
            _ok(L.kge_shard_requests(d_h.data_ptr(), d_t.data_ptr(), d_r.data_ptr(), n_pos, n_neg, stride, req.ptr(), None), _lib)
            want = requests_reference(h, t, n_pos, n_neg, stride)
            assert np.array_equal(req.get(), want), what
            if n_rel_neg:       # (the relation slot and the relation-corrupted negatives ask for nothing)
                assert (want.reshape(3 + n_neg, n_pos)[3 + n_neg - n_rel_neg:] == -1).all()
            srt, slot_of = check_count_and_scatter(want, chunk, W, what)
            h2, t2 = Guarded(len(h)), Guarded(len(t))
            d_slot_of = _dev(slot_of)
            _ok(L.kge_shard_remap_batch(d_h.data_ptr(), d_t.data_ptr(), n_pos, n_neg, stride, d_slot_of.data_ptr(), h2.ptr(), t2.ptr(),
                                        None), _lib)
            h2, t2 = h2.get().reshape(1 + n_neg, stride), t2.get().reshape(1 + n_neg, stride)
            hb, tb = h.reshape(1 + n_neg, stride), t.reshape(1 + n_neg, stride)
            assert (h2[:, n_pos:] == SENT).all() and (t2[:, n_pos:] == SENT).all(), what     # the unused tail of every block
            h2, t2, hb, tb = h2[:, :n_pos], t2[:, :n_pos], hb[:, :n_pos], tb[:, :n_pos]
            n_live = int((want >= 0).sum())
            assert h2.min() >= 0 and t2.min() >= 0 and h2.max() < n_live and t2.max() < n_live, what
            assert np.array_equal(srt[h2], hb) and np.array_equal(srt[t2], tb), what
            kept_h, kept_t = hb == hb[0], tb == tb[0]
            assert np.array_equal(h2[kept_h], np.broadcast_to(h2[0], h2.shape)[kept_h]), what
            assert np.array_equal(t2[kept_t], np.broadcast_to(t2[0], t2.shape)[kept_t]), what
            if n_rel_neg:
                assert kept_h[1 + n_neg - n_rel_neg:].all() and kept_t[1 + n_neg - n_rel_neg:].all()


# ---- copies: row gather, record ids, record packing -----------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_gather_rows(dim):
    """out[i, :] = table[clip(ids[i] - row_lo, 0, rows - 1), :], with ids from outside the shard on both sides (the documented
    clamp: the eight rows in front of and behind the table hold the sentinel, and no id here reaches further than those)."""
    torch, _lib, L = _env()
    rng = np.random.default_rng(dim)
    rows, row_lo, pad = 126, 882, 8
    alloc = torch.full(((rows + 2 * pad), dim), SENT, dtype=torch.int32, device="cuda")
    table = alloc[pad:pad + rows]
    values = rng.integers(1, 1 << 30, (rows, dim)).astype(np.int32)        # (bit patterns: the gather is a copy)
    table.copy_(torch.from_numpy(values))
    for n in (1, 1000):
        ids = rng.integers(row_lo, row_lo + rows, n)
        if n > 1:
            ids[:6] = [row_lo, row_lo + rows - 1, row_lo - 1, row_lo - pad, row_lo + rows, row_lo + rows + pad - 1]
        out, d_ids = Guarded(n, dim), _dev(ids)
        _ok(L.kge_shard_gather_rows(table.data_ptr(), d_ids.data_ptr(), n, row_lo, rows, dim, out.ptr(), None), _lib)
        assert np.array_equal(out.get(), values[np.clip(ids - row_lo, 0, rows - 1)]), (dim, n)
    torch.cuda.synchronize()
    assert (alloc[:pad] == SENT).all() and (alloc[pad + rows:] == SENT).all()


@pytest.mark.parametrize("n_records", [1, 257, 140_000])
def test_record_ids(n_records):
    """ids[m] = cache_ids[dst[m]] where dst[m] is a fetched-row slot, else -1 (no record, a relation row, a row past both)."""
    torch, _lib, L = _env()
    rng = np.random.default_rng(n_records)
    cache_rows, R = 777, 40
    cache_ids = rng.integers(0, 50_000_000, cache_rows)
    dst = rng.integers(-1, cache_rows + R + 50, n_records)
    dst[rng.random(n_records) < 0.3] = -1
    if n_records > 4:
        dst[:4] = [0, cache_rows - 1, cache_rows, cache_rows + R]
    ids, d_dst, d_cache_ids = Guarded(n_records), _dev(dst), _dev(cache_ids)
    _ok(L.kge_shard_record_ids(d_dst.data_ptr(), n_records, cache_rows, d_cache_ids.data_ptr(), ids.ptr(), None), _lib)
    slot = (dst >= 0) & (dst < cache_rows)
    assert np.array_equal(ids.get(), np.where(slot, cache_ids[np.where(slot, dst, 0)], -1))


@pytest.mark.parametrize("dim", DIMS + SCALAR_DIMS)
def test_pack_records(dim):
    """out[slot_of[m], :] = rec[m, :] for slot_of[m] >= 0; output rows no record is sent to stay as they were.  (The packing copies
    dwords whatever they hold, so the scalar widths ride along: their record size is what is checked for them.)"""
    torch, _lib, L = _env()
    rng = np.random.default_rng(dim + 1)
    dw = RECORD_DWORDS[dim]
    assert int(L.kge_transe_record_dwords(ctypes.byref(_desc(_lib, 10, 10, dim)))) == dw
    for M in (1, 1237):
        rec, _ = make_records(rng, M, dim)
        n_out = M + 5
        slot_of = np.full(M, -1, np.int64)
        travels = rng.random(M) < 0.7 if M > 1 else np.array([True])
        slot_of[travels] = rng.permutation(n_out)[:int(travels.sum())]
        out, d_rec, d_slot_of = Guarded(n_out, dw), _dev(rec), _dev(slot_of)
        _ok(L.kge_shard_pack_records(d_rec.data_ptr(), d_slot_of.data_ptr(), M, dw, out.ptr(), None), _lib)
        want = np.full((n_out, dw), SENT, np.int32)
        want[slot_of[travels]] = rec[travels]
        assert np.array_equal(out.get(), want), (dim, M)


# ---- relation count image: the atomic kernel and the sort + segmented sum + scatter route -------------------------------------

def relation_images(rec, vals, dst, cache_rows, R, past, dim):
    """(image by kge_shard_relation_counts, image by kge_transe_reduce_records + kge_shard_scatter_count_rows, numpy image)."""
    torch, _lib, L = _env()
    M, dw = rec.shape
    d_rec, d_dst = _dev(rec), _dev(dst)
    a = Guarded(R, dim); a.t.zero_()
    _ok(L.kge_shard_relation_counts(d_rec.data_ptr(), d_dst.data_ptr(), M, cache_rows, R, dw, dim, a.ptr(), None), _lib)
    # the route: every record reduced over a row space that holds all destinations, the rows of [cache_rows, cache_rows + R) scattered
    desc = _desc(_lib, cache_rows, R + past, dim)
    rows, row_counts, n_rows = Guarded(M), Guarded(M, dim), Guarded(1)
    keys = d_dst.clone()                                                         # (the reduce rewrites its keys in place)
    _ok(L.kge_transe_reduce_records(ctypes.byref(desc), d_rec.data_ptr(), keys.data_ptr(), M, rows.ptr(), row_counts.ptr(), n_rows.ptr(),
                                    None), _lib)
    b = Guarded(R, dim); b.t.zero_()
    _ok(L.kge_shard_scatter_count_rows(rows.ptr(), row_counts.ptr(), n_rows.ptr(), M, cache_rows, R, dim, b.ptr(), None), _lib)
    rows.get(); row_counts.get(); n_rows.get()
    want = np.zeros((R, dim), np.int64)
    r_rows, r_sums = sums_by_row(vals, dst, (dst >= cache_rows) & (dst < cache_rows + R))
    want[r_rows - cache_rows] = r_sums
    return a.get(), b.get(), want


@pytest.mark.parametrize("dim", DIMS)
def test_relation_count_image(dim):
    """Both ways to the dense [R, dim] image equal the numpy sum of the int8 rows by relation, and so each other; records without a
    destination, on fetched-row slots and on rows past cache_rows + R contribute nothing."""
    rng = np.random.default_rng(dim + 2)
    cache_rows, R, past, M = 300, 23, 9, 3001
    rec, vals = make_records(rng, M, dim)
    kind = rng.integers(0, 4, M)
    dst = np.select([kind == 0, kind == 1, kind == 2],
                    [np.full(M, -1), rng.integers(0, cache_rows, M), rng.integers(cache_rows, cache_rows + R, M)],
                    rng.integers(cache_rows + R, cache_rows + R + past, M))
    dst[:4] = [cache_rows - 1, cache_rows, cache_rows + R - 1, cache_rows + R]
    a, b, want = relation_images(rec, vals, dst, cache_rows, R, past, dim)
    assert np.abs(want).max() > 63                                               # (sums of many records, not single ones)
    assert np.array_equal(a, want), dim
    assert np.array_equal(b, want), dim


def test_relation_count_image_of_a_hub_relation():
    """200 000 records at dim 16, all on ONE relation row (200 000 x 63 stays inside int32)."""
    rng = np.random.default_rng(16)
    dim, M, cache_rows, R = 16, 200_000, 1000, 5
    RECORD_DWORDS.setdefault(16, 16)
    rec, vals = make_records(rng, M, dim)
    vals_biased = np.abs(vals)                       # all of one sign: the sums really reach the millions
    rec = np.zeros((M, 64), np.int8); rec[:, :dim] = vals_biased
    rec = rec.view(np.int32).reshape(M, 16)
    dst = np.full(M, cache_rows + 3)
    a, b, want = relation_images(rec, vals_biased, dst, cache_rows, R, 0, dim)
    assert want[3].min() > 1_000_000 and (np.delete(want, 3, axis=0) == 0).all()
    assert np.array_equal(a, want) and np.array_equal(b, want)


# ---- kge_transe_reduce_records ---------------------------------------------------------------------------------------------------

def check_reduce(rng, n_records, dim, n_rows_space):
    torch, _lib, L = _env()
    E = n_rows_space - 3
    desc = _desc(_lib, E, 3, dim)
    cap = max(n_records, 1)
    rows, row_counts, n_rows = Guarded(cap), Guarded(cap, dim), Guarded(1)
    if n_records == 0:
        dummy = _dev(np.zeros(16))
        _ok(L.kge_transe_reduce_records(ctypes.byref(desc), dummy.data_ptr(), dummy.data_ptr(), 0, rows.ptr(), row_counts.ptr(),
                                        n_rows.ptr(), None), _lib)
        assert n_rows.get()[0] == 0
        assert (rows.get() == SENT).all() and (row_counts.get() == SENT).all()
        return
    rec, vals = make_records(rng, n_records, dim)
    dst = rng.integers(0, n_rows_space, n_records)
    dst[rng.random(n_records) < 0.15] = -1
    dst[0] = n_rows_space - 1                                                    # the last row of the space has a record
    d_rec, d_dst = _dev(rec), _dev(dst)
    _ok(L.kge_transe_reduce_records(ctypes.byref(desc), d_rec.data_ptr(), d_dst.data_ptr(), n_records, rows.ptr(), row_counts.ptr(),
                                    n_rows.ptr(), None), _lib)
    want_rows, want_sums = sums_by_row(vals, dst, dst >= 0)
    n = int(n_rows.get()[0])
    got_rows = rows.get()[:n]          # (behind the first n rows both buffers are the reduce's to use: "sized for n_records rows")
    assert n == len(want_rows), (n_records, dim, n, len(want_rows))
    assert (np.diff(got_rows) > 0).all() and np.array_equal(got_rows, want_rows), (n_records, dim)
    assert np.array_equal(row_counts.get()[:n], want_sums), (n_records, dim)


@pytest.mark.parametrize("dim", DIMS)
def test_reduce_records(dim):
    """d_rows[:n] strictly increasing and np.unique of the live destinations, d_row_counts[:n] the exact sums, *d_n_rows = n; with
    1 .. 4097 records over few enough rows that a row's records straddle the 64-record chunks of the sorted list, and with none."""
    rng = np.random.default_rng(dim + 3)
    for n_records in (0, 1, 63, 64, 65, 4097):
        check_reduce(rng, n_records, dim, max(4, n_records // 40))
        check_reduce(rng, n_records, dim, 4 + 2 * n_records)                     # most rows hold one record


@pytest.mark.parametrize("dim", [48, 512])
def test_reduce_records_of_a_large_step(dim):
    check_reduce(np.random.default_rng(dim + 4), 100_000, dim, 2500)


# ---- which rows the row-list updates move ------------------------------------------------------------------------------------------

def _tables(rng, E, R, dim):
    """Three (entity, relation) table pairs -- parameters and two moment tables -- as Guarded allocations of float32 bit patterns."""
    out = []
    for scale, positive in ((1.0, False), (0.01, False), (1e-4, True)):
        pair = []
        for n in (E, R):
            x = (rng.standard_normal((n, dim)) * scale).astype(np.float32)
            pair.append(Guarded(n, dim).put((np.abs(x) if positive else x).view(np.int32)))
        out.append(pair)
    return out


def _row_list(rng, E, R, dim):
    """A row list as kge_transe_reduce_records leaves it: n ascending rows (entity rows, then relation rows E + r) with their
    counts, in buffers of max_rows > n entries whose tail holds valid row ids that must not be touched."""
    ent = np.sort(rng.choice(E, E // 3, replace=False))
    rel = E + np.sort(rng.choice(R, R // 2, replace=False))
    listed = np.concatenate([ent, rel])
    n = len(listed)
    unlisted = np.setdiff1d(np.arange(E + R), listed)
    tail = unlisted[:7]
    rows = np.concatenate([listed, tail])
    counts = rng.integers(-30, 31, (len(rows), dim))
    counts[:, 0] = 7                                        # (no all-zero count row: every processed row really moves)
    return listed, n, _dev(rows), _dev(counts), _dev([n]), len(rows)


def _split(listed, E):
    return listed[listed < E], listed[listed >= E] - E


@pytest.mark.parametrize("dim", [48, 200, 512])
def test_apply_rows_sgd_moves_the_listed_rows_only(dim):
    torch, _lib, L = _env()
    rng = np.random.default_rng(dim + 5)
    E, R = 211, 17
    (ent, rel), _, _ = _tables(rng, E, R, dim)
    before = ent.get(), rel.get()
    listed, n, d_rows, d_counts, d_n, max_rows = _row_list(rng, E, R, dim)
    desc = _desc(_lib, E, R, dim)
    _ok(L.kge_transe_apply_rows_sgd(ctypes.byref(desc), ent.ptr(), rel.ptr(), d_rows.data_ptr(), d_counts.data_ptr(), d_n.data_ptr(),
                                    max_rows, 100, 0.5, None), _lib)
    for got, was, moved in zip((ent.get(), rel.get()), before, _split(listed, E)):
        kept = np.setdiff1d(np.arange(len(was)), moved)
        assert np.array_equal(got[kept], was[kept]), dim
        assert (got[moved] != was[moved]).any(axis=1).all(), dim


@pytest.mark.parametrize("dim", [48, 200, 512])
def test_lazy_adam_rows_and_the_live_mask(dim):
    """kge_transe_apply_rows_adam_lazy with its d_row_live argument: rows that are not listed, and listed rows whose live flag is
    0, keep their parameter row and both moment rows bit for bit; listed live rows equal the same call made without a mask; the
    mask holds for the call it is given to (the next call without it moves every listed row)."""
    torch, _lib, L = _env()
    rng = np.random.default_rng(dim + 6)
    E, R = 211, 17
    seed_tables = _tables(rng, E, R, dim)
    start = [[g.get() for g in pair] for pair in seed_tables]
    listed, n, d_rows, d_counts, d_n, max_rows = _row_list(rng, E, R, dim)
    live = (rng.random(max_rows) < 0.5).astype(np.int32)
    live[[0, n - 1]] = [0, 1]
    live[n:] = 1                                            # (flags behind the list: nothing there is listed)
    d_live = _dev(live)
    desc = _desc(_lib, E, R, dim)

    def run(mask):
        tabs = [[Guarded(*x.shape).put(x) for x in pair] for pair in start]
        (p, p2), (m, m2), (v, v2) = tabs
        _ok(L.kge_transe_apply_rows_adam_lazy(ctypes.byref(desc), p.ptr(), p2.ptr(), m.ptr(), m2.ptr(), v.ptr(), v2.ptr(), d_rows.data_ptr(),
                                              d_counts.data_ptr(), d_n.data_ptr(), max_rows, 100, 0.01, 0.9, 0.999, 1e-8,
                                              d_live.data_ptr() if mask else None, None), _lib)
        return [[g.get() for g in pair] for pair in tabs]

    plain = run(False)
    masked = run(True)
    after = run(False)                                      # the call after the masked one: no mask any more
    moved_all = _split(listed, E)
    moved_live = _split(listed[live[:n] != 0], E)
    for k in range(3):                                      # parameters, first moments, second moments
        for side in range(2):                               # entity table, relation table
            was, full, part = start[k][side], plain[k][side], masked[k][side]
            rows_all = np.arange(len(was))
            kept = np.setdiff1d(rows_all, moved_all[side])
            assert np.array_equal(full[kept], was[kept]), (dim, k, side)
            assert (full[moved_all[side]] != was[moved_all[side]]).any(axis=1).all(), (dim, k, side)
            still = np.setdiff1d(rows_all, moved_live[side])
            assert np.array_equal(part[still], was[still]), (dim, k, side)
            assert np.array_equal(part[moved_live[side]], full[moved_live[side]]), (dim, k, side)
            assert np.array_equal(after[k][side], full), (dim, k, side)


def _tiny_lazy_case(dim):
    """TransE E = 6, R = 3: parameter, first- and second-moment tables (as numpy), a list of 4 rows (two entity rows, two relation
    rows) with non-zero counts, and a function that applies kge_transe_apply_rows_adam_lazy to fresh copies of the tables."""
    torch, _lib, L = _env()
    rng = np.random.default_rng(900 + dim)
    E, R = 6, 3
    start = [[(np.abs(x) if positive else x).astype(np.float32).view(np.int32)
              for x in (rng.standard_normal((n, dim)) * scale for n in (E, R))]
             for scale, positive in ((1.0, False), (0.01, False), (1e-4, True))]
    listed = np.array([1, 4, E + 0, E + 2])
    d_rows, d_n = _dev(listed), _dev([4])
    d_counts = _dev(rng.integers(1, 20, (4, dim)) * rng.choice([-1, 1], (4, dim)))
    desc = _desc(_lib, E, R, dim)

    def fresh():
        return [[Guarded(*x.shape).put(x) for x in pair] for pair in start]

    def apply(tabs, max_rows, d_live):
        (p, p2), (m, m2), (v, v2) = tabs
        _ok(L.kge_transe_apply_rows_adam_lazy(ctypes.byref(desc), p.ptr(), p2.ptr(), m.ptr(), m2.ptr(), v.ptr(), v2.ptr(), d_rows.data_ptr(),
                                              d_counts.data_ptr(), d_n.data_ptr(), max_rows, 100, 0.01, 0.9, 0.999, 1e-8,
                                              d_live.data_ptr() if d_live is not None else None, None), _lib)

    def read(tabs):
        return [np.concatenate([g.get() for g in pair]) for pair in tabs]      # rows of the [(E + R), D] space, as the list names them

    return listed, [np.concatenate(pair) for pair in start], fresh, apply, read


@pytest.mark.parametrize("dim", [4, 6])       # (a vector team and a scalar team)
def test_lazy_adam_row_mask_is_an_argument(dim):
    """live = [1, 0, 1, 0] over a list of 4 rows: listed rows 1 and 3 and their moments stay bit for bit, listed rows 0 and 2 equal
    the unmasked call on a copy of the tables."""
    listed, start, fresh, apply, read = _tiny_lazy_case(dim)
    plain, masked = fresh(), fresh()
    apply(plain, 4, None)
    apply(masked, 4, _dev([1, 0, 1, 0]))
    for k, (was, full, part) in enumerate(zip(start, read(plain), read(masked))):      # parameters, first moments, second moments
        assert (full[listed] != was[listed]).any(axis=1).all(), (dim, k)
        assert np.array_equal(part[listed[[1, 3]]], was[listed[[1, 3]]]), (dim, k)
        assert np.array_equal(part[listed[[0, 2]]], full[listed[[0, 2]]]), (dim, k)
        rest = np.setdiff1d(np.arange(len(was)), listed)
        assert np.array_equal(part[rest], was[rest]) and np.array_equal(full[rest], was[rest]), (dim, k)


@pytest.mark.parametrize("dim", [4, 6])
def test_lazy_adam_row_mask_of_an_empty_call_does_not_linger(dim):
    """A call with max_rows = 0 returns before its launch; the mask it was given must not reach the next, unmasked call of 4 rows:
    all four rows move, exactly as without the empty call."""
    listed, start, fresh, apply, read = _tiny_lazy_case(dim)
    plain, after_empty = fresh(), fresh()
    apply(plain, 4, None)
    apply(after_empty, 0, _dev([1, 0, 1, 0]))
    assert all(np.array_equal(a, b) for a, b in zip(read(after_empty), start))
    apply(after_empty, 4, None)
    for k, (was, full, got) in enumerate(zip(start, read(plain), read(after_empty))):
        assert (got[listed] != was[listed]).any(axis=1).all(), (dim, k)
        assert np.array_equal(got, full), (dim, k)
