"""kge_transh_emit_records_shared_chunks alone: hand-made chunk tables and candidate / pair lists (built as
tests/test_gpu_shared_emit_chunks.py builds them, every chunk of ONE relation) against the fp64 restatement of the definition
(tests/shared_transh_ref.py), and against the existing kge_forward_backward_records on the expanded batch.

Keys are exact; the loss is within 1e-5; the records summed per row are within 1e-5 of the largest element of that table's summed
gradient (the project's parity bar, RTOL of tests/test_gpu_lazy_rows.py / test_gpu_models.py).

A sign or a hinge decision must not hang on fp32 rounding, and every test asserts that in fp64 before it looks at the device:
  sign condition  no element |e| < 1e-6 in any scored triple
  kink condition  no unmasked pair with |v| < 1e-5
(the thresholds of tests/test_gpu_shared_step.py).  The tables are found by a short search on the CPU.  Random dense tables meet
the sign condition only while a case scores a few ten thousand elements (a normalised element is about 1 / sqrt(D), so a share
of about 2e-5 sqrt(D / 200) of all elements lies within 1e-6 of zero), so the larger cases take STRUCTURED tables: the lattice
entity and relation rows of tests/test_gpu_shared_emit.py, and normal vectors with two (D < 16) or four elements +-1 and zeros
elsewhere.  The projection then moves a row's elements at those positions onto multiples of 0.05 or 0.1 and leaves the others
alone, the norms change by less than 1 %, and no signed sum x^ + r^ - y^ comes closer to zero than about 0.1 / sqrt(D) -- while a,
d and the normal vector's gradient take all their terms.  Every case here finds its tables, so no row is excused."""
import ctypes
import functools

import numpy as np
import pytest

import shared_transh_ref as tref
from test_gpu_shared_emit import E, MARGIN, R, SHAPES, lattice_tables
from test_gpu_shared_emit_chunks import make_lists, table_of

pytestmark = pytest.mark.gpu

DIMS = [4, 50, 200, 260, 512]
RTOL = 1e-5
N_POS_TOTAL = 960          # the step the call is a part of: (2 * 960) // (2 R 64) = 3 hub copies, so the keys use j % 3
TRANSH = 1


def dense_tables(D, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.1, (E, D)).astype(np.float32), rng.normal(0, 0.1, (R, D)).astype(np.float32),
            rng.normal(0, 1.0, (R, D)).astype(np.float32))


def structured_tables(D, seed):
    ent, rel = lattice_tables(D, seed)
    rng = np.random.default_rng(seed + 77)
    nrm = np.zeros((R, D), dtype=np.float32)
    for i in range(R):
        at = rng.choice(D, 2 if D < 16 else 4, replace=False)
        nrm[i, at] = rng.choice([-1.0, 1.0], len(at)) * 0.6
    return ent, rel, nrm


def lists_for(P, N, seed, mask):
    """Chunks of length P, 1, P - 1 (where that is a length), P, 1, then two empty slots; chunk j has relation j % R."""
    lens = [P, 1] + ([P - 1] if P >= 2 else []) + [P, 1]
    chunks, n_pos = table_of(lens)
    h, t, r, cand, pair = make_lists(n_pos, len(chunks), N, seed, mask=mask)
    for j, (lo, n) in enumerate(chunks.tolist()):
        r[lo:lo + n] = j % R
    if not mask:      # the expanded batch must be sampler-shaped: a candidate may not be the entity it replaces
        c = cand[tref.chunk_of_positions(chunks, n_pos)]
        same = np.where(pair & 1, c == h[:, None], c == t[:, None])
        pair[same] ^= 1
        assert not np.where(pair & 1, c == h[:, None], c == t[:, None]).any()
    return chunks, n_pos, h, t, r, cand, pair


@functools.lru_cache(maxsize=None)
def case(D, P, N, mask=True, zero_normal=False):
    """The first tables and lists of a short search that meet the sign and the kink condition in fp64, with the reference."""
    tried = []
    n_scored = None
    for kind, make, seeds in (("dense", dense_tables, range(4)), ("structured", structured_tables, range(16))):
        for seed in seeds:
            chunks, n_pos, h, t, r, cand, pair = lists_for(P, N, 1000 * D + 10 * P + N + 7919 * seed, mask)
            n_scored = n_pos * (N + 1) * D
            if kind == "dense" and n_scored > 100000:
                break
            ent, rel, nrm = make(D, 31 * D + P + seed)
            if zero_normal:
                nrm[3] = 0.0      # chunk 3 (length P): the clipped normalise makes its projection the identity
            denom = n_pos * N
            want = tref.forward(ent, rel, nrm, h, t, r, cand, pair, chunks, MARGIN, denom, N_POS_TOTAL)
            tried.append((kind, seed, want["min_sign"], want["min_kink"]))
            if want["min_sign"] >= 1e-6 and want["min_kink"] >= 1e-5:
                return dict(kind=kind, seed=seed, ent=ent, rel=rel, nrm=nrm, h=h, t=t, r=r, cand=cand, pair=pair, chunks=chunks,
                            n_pos=n_pos, denom=denom, want=want)
    raise AssertionError("no tables meet the conditions: %r" % (tried,))


def desc_for(D, model=TRANSH):
    from openkeonspark_amd import _lib
    d = _lib.ModelDesc()
    d.model = model; d.negative_rel = 0; d.ent_total = E; d.rel_total = R; d.ent_dim = D; d.rel_dim = D; d.margin = MARGIN
    return d


def run_emit(L, desc, c, stride):
    import torch
    from openkeonspark_amd import _lib
    n_pos, (cap, N) = c["n_pos"], c["cand"].shape
    D = c["ent"].shape[1]
    M = 2 * n_pos + cap * (N + 2)
    dev = lambda a, n: torch.from_numpy(np.concatenate([a, np.zeros(n - len(a), a.dtype)])).cuda()
    dh, dt, dr = dev(c["h"], stride), dev(c["t"], stride), dev(c["r"], stride)
    tabs = [torch.from_numpy(c[k]).cuda() for k in ("ent", "rel", "nrm")]
    dc, dp, dtab = torch.from_numpy(c["cand"]).cuda(), torch.from_numpy(c["pair"]).cuda(), torch.from_numpy(np.ascontiguousarray(c["chunks"])).cuda()
    rec = torch.full((M + 1, D), 7.25, dtype=torch.float32, device="cuda")
    dst = torch.full((M + 1,), -7, dtype=torch.int32, device="cuda")
    loss = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    rc = L.kge_transh_emit_records_shared_chunks(ctypes.byref(desc), _lib.table_ptrs([x.data_ptr() for x in tabs]), dh.data_ptr(), dt.data_ptr(),
                                                 dr.data_ptr(), n_pos, stride, dtab.data_ptr(), cap, dc.data_ptr(), N, dp.data_ptr(), c["denom"],
                                                 N_POS_TOTAL, rec.data_ptr(), dst.data_ptr(), loss.data_ptr(), None)
    assert rc == 0, _lib.last_error(L)
    torch.cuda.synchronize()
    assert int(dst[M].item()) == -7 and (rec[M] == 7.25).all()      # nothing past the last record
    return rec[:M].cpu().numpy(), dst[:M].cpu().numpy().astype(np.int64), float(loss.item())


def assert_gradients_agree(got, want, what):
    for name in want:
        scale = np.abs(want[name]).max()
        off = np.abs(got[name] - want[name]).max()
        print("   %s %s: largest element %.3e, largest difference %.3e (bound %.3e)" % (what, name, scale, off, RTOL * scale))
        assert off <= RTOL * scale, (what, name, off, scale)


@pytest.fixture(scope="module")
def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


CASES = [(D, P, N, False) for D in DIMS for P, N in SHAPES] + [(50, 2, 63, True), (200, 64, 25, True)]


@pytest.mark.parametrize("D,P,N,zero_normal", CASES)
def test_records_equal_the_definition(lib, D, P, N, zero_normal):
    c = case(D, P, N, True, zero_normal)
    want, n_pos, cap = c["want"], c["n_pos"], len(c["chunks"])
    assert want["min_sign"] >= 1e-6 and want["min_kink"] >= 1e-5      # before the device is looked at
    rec, keys, loss = run_emit(lib, desc_for(D), c, n_pos + 5)
    print("D %d P %d N %d (%s tables, seed %d) n_pos %d cap %d: active %d of %d pairs, loss %.6f (fp64 %.6f), min kink %.2e, min sign %.2e"
          % (D, P, N, c["kind"], c["seed"], n_pos, cap, int(want["active"].sum()), n_pos * N, loss, want["loss"], want["min_kink"],
             want["min_sign"]))
    assert n_pos * N < 20 or want["active"].any()
    assert np.array_equal(keys, want["keys"])
    m_c0 = 2 * n_pos + 2 * cap
    for j in (cap - 2, cap - 1):      # the empty slots: no relation record, no normal-vector record, no candidate
        assert keys[2 * n_pos + j] == -1 and keys[2 * n_pos + cap + j] == -1 and (keys[m_c0 + j * N:m_c0 + (j + 1) * N] == -1).all()
    assert n_pos * N < 20 or len(set(((keys[keys >= E] - E) // (2 * R)).tolist())) > 1      # more than one hub copy is keyed
    assert abs(loss - want["loss"]) <= 1e-5 * abs(want["loss"])
    got = tref.table_gradients(keys, rec, E, R, N_POS_TOTAL)
    assert_gradients_agree(got, tref.table_gradients(want["keys"], want["records"], E, R, N_POS_TOTAL), "fp64")
    if zero_normal:
        # relation 3's normal vector is zero: its gradient is the clipped backward of an accumulator that is exactly zero
        assert 3 in tref.touched_rows(keys, E, R, N_POS_TOTAL)["normal_vectors"] and not got["normal_vectors"][3].any()


@pytest.mark.parametrize("D,P,N", [(D, P, N) for D in DIMS for P, N in SHAPES])
def test_the_unshared_kernel_on_the_expanded_batch_agrees(lib, D, P, N):
    """The same lists without masks, spelled out as an ordinary batch, through kge_forward_backward_records for TransH: per row the
    two kernels' records sum to the same gradient."""
    import torch
    from openkeonspark_amd import _lib
    c = case(D, P, N, False)
    want, n_pos = c["want"], c["n_pos"]
    assert want["min_sign"] >= 1e-6 and want["min_kink"] >= 1e-5
    desc = desc_for(D)
    rec, keys, loss = run_emit(lib, desc, c, n_pos + 3)
    bh, bt, br = tref.expand(c["h"], c["t"], c["r"], c["cand"], c["pair"], c["chunks"], n_pos)
    M2 = n_pos * (4 + N)
    tabs = [torch.from_numpy(c[k]).cuda() for k in ("ent", "rel", "nrm")]
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
    got = tref.table_gradients(keys, rec, E, R, N_POS_TOTAL)
    other = tref.table_gradients(dst2.cpu().numpy(), rec2.cpu().numpy(), E, R, N_POS_TOTAL)
    assert any(np.abs(v).max() > 0 for v in other.values()) or n_pos * N < 20
    assert_gradients_agree(got, other, "unshared")


def test_refusals(lib):
    """The entry point's refusals, with their words; a missing table or chunk table is a bad argument."""
    import torch
    from openkeonspark_amd import _lib
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    f = torch.zeros((E + R, 1024), dtype=torch.float32, device="cuda")
    table = torch.tensor([[0, 1]], dtype=torch.int32, device="cuda")
    all_tabs = [f.data_ptr()] * 3

    def call(desc, N, tab=table.data_ptr(), cap=1, tabs=all_tabs):
        return lib.kge_transh_emit_records_shared_chunks(ctypes.byref(desc), _lib.table_ptrs(tabs), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                                         1, 1, tab, cap, z.data_ptr(), N, z.data_ptr(), 1, 1, f.data_ptr(), z.data_ptr(),
                                                         f.data_ptr(), None)

    for change, N, word in ((dict(model=0), 2, "TransE"), (dict(model=3), 2, "TransD"), (dict(negative_rel=1), 2, "negative_rel"),
                            ({}, 64, "63"), (dict(ent_dim=516, rel_dim=516), 2, "512")):
        d = desc_for(8)
        for k, v in change.items():
            setattr(d, k, v)
        assert call(d, N) == -4
        assert word in _lib.last_error(lib)
        assert lib.kge_shared_float_supported(ctypes.byref(d), N) == 0
    assert call(desc_for(8), 2, tabs=[f.data_ptr(), f.data_ptr()]) < 0 and "table" in _lib.last_error(lib)      # no normal_vectors
    assert call(desc_for(8), 2, tab=None) < 0
    assert call(desc_for(8), 2, cap=0) < 0
    assert lib.kge_shared_float_supported(ctypes.byref(desc_for(8)), 2) == 1
    assert call(desc_for(8), 2) == 0
    torch.cuda.synchronize()
