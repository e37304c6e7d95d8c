"""kge_transd_emit_records_shared_chunks alone: the hand-made chunk tables and candidate / pair lists of
tests/test_gpu_shared_transh_emit.py (lengths P, 1, P - 1, P, 1 and two empty slots, every chunk of ONE relation; a repeated
candidate, a positive's own head as new tail, ids -1 and E + 3, a fully masked positive, random masks) against the fp64 restatement
of the definition (tests/shared_transd_ref.py), and against the existing kge_forward_backward_records for TransD on the expanded
batch.

Keys are exact; the loss is within 1e-5; the records summed per row are within 1e-5 of the largest element of that table's summed
gradient, for each of the four tables (the bounds of the TransH kernel's test).

A sign or a hinge decision must not hang on fp32 rounding, and every test asserts that in fp64 before it looks at the device:
  sign condition  no element |e| < 1e-6 in any scored triple
  kink condition  no unmasked pair with |v| < 1e-5
The tables are found by a short search on the CPU: dense random tables while a case scores few elements, and beyond that the
lattice entity and relation rows of tests/test_gpu_shared_emit.py with SPARSE transfer vectors -- two (D < 16) or four elements
+-0.6 and zeros elsewhere in every ent_transfer and rel_transfer row.  a = x . x_p is then a multiple of 0.12 and the projection
moves the elements of x at r_p's positions by multiples of 0.072, which never meets a lattice value of +-0.1 or +-0.3, while a, d
and both transfer gradients take all their terms.  Every case here finds its tables, so no row is excused.

Width 258 takes the <2, false> instantiation (eight elements per lane, scalar accesses); (2, 63) from width 200 on and (64, 25)
at width 512 run more than one candidate tile, where a positive's count vectors wait in its record slots."""
import ctypes
import functools

import numpy as np
import pytest

import shared_transd_ref as dref
from test_gpu_shared_emit import E, MARGIN, R, SHAPES, lattice_tables
from test_gpu_shared_transh_emit import N_POS_TOTAL, RTOL, assert_gradients_agree, desc_for, lists_for

pytestmark = pytest.mark.gpu

DIMS = [4, 50, 200, 258, 260, 512]
TRANSD = 3
NAMES = ("ent", "rel", "relp", "entp")      # the order of the kernel's tables


def dense_tables(D, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.1, (E, D)).astype(np.float32), rng.normal(0, 0.1, (R, D)).astype(np.float32),
            rng.normal(0, 0.3, (R, D)).astype(np.float32), rng.normal(0, 0.3, (E, D)).astype(np.float32))


def sparse_rows(rng, rows, D):
    out = np.zeros((rows, D), dtype=np.float32)
    for i in range(rows):
        at = rng.choice(D, 2 if D < 16 else 4, replace=False)
        out[i, at] = rng.choice([-1.0, 1.0], len(at)) * 0.6
    return out


def structured_tables(D, seed):
    ent, rel = lattice_tables(D, seed)
    rng = np.random.default_rng(seed + 77)
    return ent, rel, sparse_rows(rng, R, D), sparse_rows(rng, E, D)


@functools.lru_cache(maxsize=None)
def case(D, P, N, mask=True, zero_transfer=False):
    """The first tables and lists of a short search that meet the sign and the kink condition in fp64, with the reference."""
    tried = []
    for kind, make, seeds in (("dense", dense_tables, range(4)), ("structured", structured_tables, range(16))):
        for seed in seeds:
            chunks, n_pos, h, t, r, cand, pair = lists_for(P, N, 1000 * D + 10 * P + N + 7919 * seed, mask)
            if kind == "dense" and n_pos * (N + 1) * D > 100000:
                break
            ent, rel, relp, entp = make(D, 31 * D + P + seed)
            if zero_transfer:
                relp[3] = 0.0      # chunk 3 (length P): the projection is the identity, d = 0, zero transfer records WITH keys
            denom = n_pos * N
            want = dref.forward(ent, rel, relp, entp, h, t, r, cand, pair, chunks, MARGIN, denom, N_POS_TOTAL)
            tried.append((kind, seed, want["min_sign"], want["min_kink"]))
            if want["min_sign"] >= 1e-6 and want["min_kink"] >= 1e-5:
                return dict(kind=kind, seed=seed, ent=ent, rel=rel, relp=relp, entp=entp, h=h, t=t, r=r, cand=cand, pair=pair,
                            chunks=chunks, n_pos=n_pos, denom=denom, want=want)
    raise AssertionError("no tables meet the conditions: %r" % (tried,))


def run_emit(L, desc, c, stride):
    import torch
    from openkeonspark_amd import _lib
    n_pos, (cap, N) = c["n_pos"], c["cand"].shape
    D = c["ent"].shape[1]
    M = 4 * n_pos + cap * (2 * N + 2)
    dev = lambda a, n: torch.from_numpy(np.concatenate([a, np.zeros(n - len(a), a.dtype)])).cuda()
    dh, dt, dr = dev(c["h"], stride), dev(c["t"], stride), dev(c["r"], stride)
    tabs = [torch.from_numpy(c[k]).cuda() for k in NAMES]
    dc, dp, dtab = torch.from_numpy(c["cand"]).cuda(), torch.from_numpy(c["pair"]).cuda(), torch.from_numpy(np.ascontiguousarray(c["chunks"])).cuda()
    rec = torch.full((M + 1, D), 7.25, dtype=torch.float32, device="cuda")
    dst = torch.full((M + 1,), -7, dtype=torch.int32, device="cuda")
    loss = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    rc = L.kge_transd_emit_records_shared_chunks(ctypes.byref(desc), _lib.table_ptrs([x.data_ptr() for x in tabs]), dh.data_ptr(), dt.data_ptr(),
                                                 dr.data_ptr(), n_pos, stride, dtab.data_ptr(), cap, dc.data_ptr(), N, dp.data_ptr(), c["denom"],
                                                 N_POS_TOTAL, rec.data_ptr(), dst.data_ptr(), loss.data_ptr(), None)
    assert rc == 0, _lib.last_error(L)
    torch.cuda.synchronize()
    assert int(dst[M].item()) == -7 and (rec[M] == 7.25).all()      # nothing past the last record
    return rec[:M].cpu().numpy(), dst[:M].cpu().numpy().astype(np.int64), float(loss.item())


@pytest.fixture(scope="module")
def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


CASES = [(D, P, N, False) for D in DIMS for P, N in SHAPES] + [(50, 2, 63, True), (200, 64, 25, True), (258, 2, 63, True)]


@pytest.mark.parametrize("D,P,N,zero_transfer", CASES)
def test_records_equal_the_definition(lib, D, P, N, zero_transfer):
    c = case(D, P, N, True, zero_transfer)
    want, n_pos, cap = c["want"], c["n_pos"], len(c["chunks"])
    assert want["min_sign"] >= 1e-6 and want["min_kink"] >= 1e-5      # before the device is looked at
    rec, keys, loss = run_emit(lib, desc_for(D, TRANSD), c, n_pos + 5)
    print("D %d P %d N %d (%s tables, seed %d) n_pos %d cap %d: active %d of %d pairs, loss %.6f (fp64 %.6f), min kink %.2e, min sign %.2e"
          % (D, P, N, c["kind"], c["seed"], n_pos, cap, int(want["active"].sum()), n_pos * N, loss, want["loss"], want["min_kink"],
             want["min_sign"]))
    assert n_pos * N < 20 or want["active"].any()
    assert np.array_equal(keys, want["keys"])
    m_c0 = 4 * n_pos + 2 * cap
    for j in (cap - 2, cap - 1):      # the empty slots: no relation records, no candidate of either table
        assert keys[4 * n_pos + j] == -1 and keys[4 * n_pos + cap + j] == -1
        assert (keys[m_c0 + j * N:m_c0 + (j + 1) * N] == -1).all() and (keys[m_c0 + (cap + j) * N:m_c0 + (cap + j + 1) * N] == -1).all()
    # an entity's transfer record has a key exactly when its row's record has one, and it is E beyond it
    for lo, n, step in ((0, n_pos, n_pos), (2 * n_pos, n_pos, n_pos), (m_c0, cap * N, cap * N)):
        k0, k1 = keys[lo:lo + n], keys[lo + step:lo + step + n]
        assert np.array_equal(k1, np.where(k0 >= 0, k0 + E, -1))
    assert n_pos * N < 20 or len(set(((keys[keys >= 2 * E] - 2 * E) // (2 * R)).tolist())) > 1      # more than one hub copy is keyed
    assert abs(loss - want["loss"]) <= 1e-5 * abs(want["loss"])
    got = dref.table_gradients(keys, rec, E, R, N_POS_TOTAL)
    assert_gradients_agree(got, dref.table_gradients(want["keys"], want["records"], E, R, N_POS_TOTAL), "fp64")
    if zero_transfer:
        # relation 3's transfer vector is zero: chunk 3's entities have d = 0, so their transfer records are zero and keyed
        lo, n = c["chunks"][3].tolist()
        slots = np.concatenate([np.arange(n_pos + lo, n_pos + lo + n), np.arange(3 * n_pos + lo, 3 * n_pos + lo + n),
                                np.arange(m_c0 + (cap + 3) * N, m_c0 + (cap + 4) * N)])
        keyed = slots[keys[slots] >= 0]
        assert len(keyed) > 0 and not rec[keyed].any()
        assert 3 in dref.touched_rows(keys, E, R, N_POS_TOTAL)["rel_transfer"]


@pytest.mark.parametrize("D,P,N", [(D, P, N) for D in DIMS for P, N in SHAPES])
def test_the_unshared_kernel_on_the_expanded_batch_agrees(lib, D, P, N):
    """The same lists without masks, spelled out as an ordinary batch, through kge_forward_backward_records for TransD: per row of
    each of the four tables the two kernels' records sum to the same gradient."""
    import torch
    from openkeonspark_amd import _lib
    c = case(D, P, N, False)
    want, n_pos = c["want"], c["n_pos"]
    assert want["min_sign"] >= 1e-6 and want["min_kink"] >= 1e-5
    desc = desc_for(D, TRANSD)
    rec, keys, loss = run_emit(lib, desc, c, n_pos + 3)
    bh, bt, br = dref.expand(c["h"], c["t"], c["r"], c["cand"], c["pair"], c["chunks"], n_pos)
    M2 = n_pos * (6 + 2 * N)
    tabs = [torch.from_numpy(c[k]).cuda() for k in NAMES]
    d3 = [torch.from_numpy(x).cuda() for x in (bh, bt, br)]
    rec2 = torch.zeros((M2, D), dtype=torch.float32, device="cuda")
    dst2 = torch.full((M2,), -1, dtype=torch.int32, device="cuda")
    loss2 = torch.zeros(1, dtype=torch.float32, device="cuda")
    rc = lib.kge_forward_backward_records(ctypes.byref(desc), _lib.table_ptrs([x.data_ptr() for x in tabs]), d3[0].data_ptr(), d3[1].data_ptr(),
                                          d3[2].data_ptr(), n_pos, N, n_pos, c["denom"], N_POS_TOTAL, rec2.data_ptr(), dst2.data_ptr(), 0, M2,
                                          loss2.data_ptr(), None)
    assert rc == 0, _lib.last_error(lib)
    torch.cuda.synchronize()
    skipped = ctypes.c_int32(-1)
    assert lib.kge_sgd_rows_skipped(ctypes.byref(skipped)) == 0 and skipped.value == 0
    loss2 = float(loss2.item())
    assert abs(loss - loss2) <= 1e-5 * abs(loss2) and abs(loss - want["loss"]) <= 1e-5 * abs(want["loss"])
    got = dref.table_gradients(keys, rec, E, R, N_POS_TOTAL)
    other = dref.table_gradients(dst2.cpu().numpy(), rec2.cpu().numpy(), E, R, N_POS_TOTAL)
    assert any(np.abs(v).max() > 0 for v in other.values()) or n_pos * N < 20
    assert_gradients_agree(got, other, "unshared")


def test_refusals(lib):
    """The entry point's refusals, with their words; a missing table or chunk table is a bad argument."""
    import torch
    from openkeonspark_amd import _lib
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    f = torch.zeros((E + R, 1024), dtype=torch.float32, device="cuda")
    table = torch.tensor([[0, 1]], dtype=torch.int32, device="cuda")
    all_tabs = [f.data_ptr()] * 4

    def call(desc, N, tab=table.data_ptr(), cap=1, tabs=all_tabs):
        return lib.kge_transd_emit_records_shared_chunks(ctypes.byref(desc), _lib.table_ptrs(tabs), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                                         1, 1, tab, cap, z.data_ptr(), N, z.data_ptr(), 1, 1, f.data_ptr(), z.data_ptr(),
                                                         f.data_ptr(), None)

    for change, N, word in ((dict(model=0), 2, "TransD"), (dict(model=1), 2, "TransD"), (dict(model=2), 2, "TransD"),
                            (dict(negative_rel=1), 2, "negative_rel"), ({}, 64, "63"), (dict(ent_dim=516, rel_dim=516), 2, "512")):
        d = desc_for(8, TRANSD)
        for k, v in change.items():
            setattr(d, k, v)
        assert call(d, N) == -4
        assert word in _lib.last_error(lib)
        assert lib.kge_shared_transd_supported(ctypes.byref(d), N) == 0
    for missing in range(4):      # a null table among the four
        tabs = list(all_tabs)
        tabs[missing] = None
        assert call(desc_for(8, TRANSD), 2, tabs=tabs) < 0 and "table" in _lib.last_error(lib)
    assert call(desc_for(8, TRANSD), 2, tab=None) < 0
    assert call(desc_for(8, TRANSD), 2, cap=0) < 0
    assert lib.kge_shared_transd_supported(ctypes.byref(desc_for(8, TRANSD)), 2) == 1
    assert lib.kge_shared_float_supported(ctypes.byref(desc_for(8, TRANSD)), 2) == 0      # the TransH entry point still refuses TransD
    assert call(desc_for(8, TRANSD), 2) == 0
    torch.cuda.synchronize()
