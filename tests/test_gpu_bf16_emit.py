"""kge_transe_emit_records_bf16 alone, by the rule of tests/test_gpu_shared_transd_emit.py: nothing is excused.

Before the device is looked at, the fp64 reference on the widened tables (tests/bf16_ref.py) must find
  sign condition  no element |e| < 1e-6 in any scored triple
  kink condition  no hinge within 1e-5 of its kink
and a short seed search on the CPU picks tables and batch that meet both.  Random normal rows cannot meet the sign condition at
these sizes, so the tables are the lattice of tests/test_gpu_shared_emit.py (an entity row a signed permutation of half 0.1 and
half 0.3, a relation row all +-0.07) rounded to bf16 -- still three magnitudes, whose signed sums after normalisation stay about
0.1 / sqrt(D) away from zero.

Then: the keys are exact; the first D bytes of every live record are exact against the fp64 reference and against
kge_transe_emit_records run on the float32 copy of the same tables; the loss is within 1e-5 relative; kge_transe_reduce_records
on the records gives the reference's per-row counts exactly.

kge_transe_emit_records itself refuses more than 63 negatives (kge_transe_counts_supported: a positive's int8 sums hold 2 x 63
signs), so at n_neg = 70 there is no fp32 run to compare with: the test asserts that refusal and keeps every other comparison."""
import ctypes
import functools

import numpy as np
import pytest

import bf16_ref as ref

pytestmark = pytest.mark.gpu

E, R, N_POS, STRIDE = 500, 7, 301, 304
MARGIN = 0.3217
TRANSE = 0
KGE_ERR_UNSUPPORTED = -4
# {8, 24, 200, 512, 1024} and one width either side of every rung boundary of csrc/team_shape.hpp that is a multiple of 8
DIMS = [8, 16, 24, 32, 40, 64, 72, 128, 136, 200, 256, 264, 512, 520, 1024]
NEGS = [1, 25, 70]


def lattice_tables(D, seed):
    rng = np.random.default_rng(seed)
    mags = np.array([1.0] * (D - D // 2) + [3.0] * (D // 2))
    ent = np.stack([rng.permutation(mags) for _ in range(E)]) * rng.choice([-1.0, 1.0], (E, D)) * 0.1
    rel = rng.choice([-1.0, 1.0], (R, D)) * 0.07
    return ref.to_bf16(ent.astype(np.float32)), ref.to_bf16(rel.astype(np.float32))


def sampler_shaped_batch(n_neg, n_rel, seed):
    """Positives and negatives in the layout of Base.cpp: every negative differs from its positive in exactly one slot; the last
    n_rel negatives of a group are relation negatives."""
    rng = np.random.default_rng(seed)
    bh, bt, br = (np.zeros(STRIDE * (1 + n_neg), np.int32) for _ in range(3))
    h = rng.integers(0, E, N_POS); t = (h + 1 + rng.integers(0, E - 1, N_POS)) % E; r = rng.integers(0, R, N_POS)
    bh[:N_POS], bt[:N_POS], br[:N_POS] = h, t, r
    for k in range(n_neg):
        s = slice((k + 1) * STRIDE, (k + 1) * STRIDE + N_POS)
        bh[s], bt[s], br[s] = h, t, r
        if k >= n_neg - n_rel:
            br[s] = (r + 1 + rng.integers(0, R - 1, N_POS)) % R
        else:
            head = rng.integers(0, 2, N_POS).astype(bool)
            bh[s] = np.where(head, (h + 1 + rng.integers(0, E - 1, N_POS)) % E, h)
            bt[s] = np.where(head, t, (t + 1 + rng.integers(0, E - 1, N_POS)) % E)
    return bh, bt, br


@functools.lru_cache(maxsize=None)
def case(D, n_neg, negative_rel):
    n_rel = min(negative_rel, n_neg)
    tried = []
    for seed in range(8):
        ent, rel = lattice_tables(D, 31 * D + n_neg + seed)
        bh, bt, br = sampler_shaped_batch(n_neg, n_rel, 1000 * D + 10 * n_neg + negative_rel + 7919 * seed)
        want = ref.emit(ref.widen(ent), ref.widen(rel), bh, bt, br, N_POS, n_neg, STRIDE, MARGIN, N_POS * n_neg)
        tried.append((seed, want["min_sign"], want["min_kink"]))
        if want["min_sign"] >= 1e-6 and want["min_kink"] >= 1e-5:
            return dict(ent=ent, rel=rel, bh=bh, bt=bt, br=br, want=want)
    raise AssertionError("no tables meet the conditions: %r" % (tried,))


def desc_for(D, negative_rel):
    from openkeonspark_amd import _lib
    return _lib.ModelDesc(TRANSE, negative_rel, E, R, D, D, MARGIN, 0)


def run_emit(c, D, n_neg, negative_rel, fp32=False):
    """-> (rc, keys, records as int8 [M, 4 dw], loss, deferred groups, the device tensors of records and keys)."""
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    desc = desc_for(D, negative_rel)
    dw = int(L.kge_transe_record_dwords(ctypes.byref(desc)))
    M = N_POS * (3 + n_neg)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bh, bt, br = d(c["bh"]), d(c["bt"]), d(c["br"])
    rec = torch.full((M, dw), 0x55555555, dtype=torch.int32, device="cuda")
    dst = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    if fp32:
        ent, rel = d(ref.widen(c["ent"])), d(ref.widen(c["rel"]))
        L.kge_set_option(b"tables_changed", 1)      # fresh tensors may reuse an address whose 1/|row| table the engine still holds
        rc = L.kge_transe_emit_records(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), bh.data_ptr(), bt.data_ptr(), br.data_ptr(),
                                       N_POS, n_neg, STRIDE, N_POS * n_neg, rec.data_ptr(), dst.data_ptr(), None, None, loss.data_ptr(), None)
    else:
        ent, rel = d(c["ent"].view(np.int16)), d(c["rel"].view(np.int16))
        rc = L.kge_transe_emit_records_bf16(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), bh.data_ptr(), bt.data_ptr(), br.data_ptr(),
                                            N_POS, n_neg, STRIDE, N_POS * n_neg, rec.data_ptr(), dst.data_ptr(), loss.data_ptr(), None)
    if rc:
        L.kge_clear_error()
        return rc, None, None, None, None, None, None
    nd = ctypes.c_int32(-1)
    _lib.check(L.kge_transe_deferred_groups(ctypes.byref(nd)), L)
    return (0, dst.cpu().numpy(), rec.cpu().numpy().view(np.int8).reshape(M, 4 * dw), float(loss.item()), nd.value, rec, dst)


@pytest.mark.parametrize("negative_rel", [0, 2])
@pytest.mark.parametrize("n_neg", NEGS)
@pytest.mark.parametrize("D", DIMS)
def test_records_keys_loss_and_counts(D, n_neg, negative_rel):
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    c = case(D, n_neg, negative_rel)
    want = c["want"]
    rc, keys, rec, loss, deferred, d_rec, d_dst = run_emit(c, D, n_neg, negative_rel)
    assert rc == 0 and deferred == want["deferred"]      # (only groups with more than 63 ACTIVE negatives: none up to n_neg = 63)
    assert n_neg > 63 or deferred == 0
    np.testing.assert_array_equal(keys, want["keys"])
    live = want["keys"] >= 0
    assert live.sum() > N_POS
    np.testing.assert_array_equal(rec[live][:, :D], want["rec"][live])
    print("loss %.9g reference %.9g relative %.3g" % (loss, want["loss"], abs(loss - want["loss"]) / abs(want["loss"])))
    assert abs(loss - want["loss"]) <= 1e-5 * abs(want["loss"])
    # ... against the fp32 kernel on the float32 copy of the same tables
    rc32, keys32, rec32, loss32, deferred32, _, _ = run_emit(c, D, n_neg, negative_rel, fp32=True)
    if n_neg > 63:
        assert rc32 == KGE_ERR_UNSUPPORTED      # (see the module's text)
    else:
        assert rc32 == 0 and deferred32 == 0
        np.testing.assert_array_equal(keys, keys32)
        np.testing.assert_array_equal(rec[live][:, :D], rec32[live][:, :D])
        assert abs(loss - loss32) <= 1e-5 * abs(loss32)
    # ... and the unchanged reduce on the records
    M = keys.shape[0]
    desc = desc_for(D, negative_rel)
    rows = torch.zeros(M, dtype=torch.int32, device="cuda")
    counts = torch.zeros((M, D), dtype=torch.int32, device="cuda")
    n_rows = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L.kge_transe_reduce_records(ctypes.byref(desc), d_rec.data_ptr(), d_dst.data_ptr(), M, rows.data_ptr(), counts.data_ptr(),
                                           n_rows.data_ptr(), None), L)
    n = int(n_rows.item())
    got_rows, got_counts = rows[:n].cpu().numpy(), counts[:n].cpu().numpy()
    order = np.argsort(got_rows)
    want_rows, want_counts = ref.row_counts(want["keys"], want["rec"])
    np.testing.assert_array_equal(got_rows[order], want_rows)
    np.testing.assert_array_equal(got_counts[order], want_counts)


@pytest.mark.parametrize("D,n_neg", [(24, 5), (200, 25), (1024, 70)])
def test_a_group_that_is_not_sampler_shaped_is_deferred(D, n_neg):
    """One hand-made group whose second negative changes head AND tail: all its keys are -1, kge_transe_deferred_groups counts it,
    it adds nothing to the loss, and every other group's keys and records are what they were."""
    c = dict(case(D, n_neg, 0))
    b = 17
    bh, bt = c["bh"].copy(), c["bt"].copy()
    j = b + min(2, n_neg) * STRIDE
    bh[j] = (c["bh"][b] + 1) % E
    bt[j] = (c["bt"][b] + 1) % E
    c.update(bh=bh, bt=bt)
    want = ref.emit(ref.widen(c["ent"]), ref.widen(c["rel"]), bh, bt, c["br"], N_POS, n_neg, STRIDE, MARGIN, N_POS * n_neg)
    assert want["deferred"] == 1 + c["want"]["deferred"] and want["min_sign"] >= 1e-6 and want["min_kink"] >= 1e-5
    rc, keys, rec, loss, deferred, _, _ = run_emit(c, D, n_neg, 0)
    assert rc == 0 and deferred == want["deferred"]
    assert (keys.reshape(3 + n_neg, N_POS)[:, b] == -1).all()
    np.testing.assert_array_equal(keys, want["keys"])
    live = want["keys"] >= 0
    np.testing.assert_array_equal(rec[live][:, :D], want["rec"][live])
    assert abs(loss - want["loss"]) <= 1e-5 * abs(want["loss"])


def test_unsupported_shapes_are_refused_with_the_reason():
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    for D, n_neg, model, why in ((100, 5, TRANSE, "multiple of 8"), (1032, 5, TRANSE, "up to 1024"), (24, 0, TRANSE, "1 to 127 negatives"),
                                 (24, 128, TRANSE, "1 to 127 negatives"), (24, 5, 1, "TransE only")):
        desc = _lib.ModelDesc(model, 0, E, R, D, D, MARGIN, 0)
        assert L.kge_bf16_tables_supported(ctypes.byref(desc), n_neg) == 0
        with pytest.raises(_lib.KgeError) as e:
            _lib.check(L.kge_transe_emit_records_bf16(ctypes.byref(desc), p, p, p, p, p, 1, n_neg, 1, 1, p, p, p, None), L)
        assert why in str(e.value)
    assert L.kge_bf16_tables_supported(ctypes.byref(_lib.ModelDesc(TRANSE, 0, E, R, 24, 24, MARGIN, 0)), 70) == 1
