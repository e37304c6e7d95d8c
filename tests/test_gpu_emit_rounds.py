"""The TransE emit kernel's round body at widths 132..256 (csrc/models.hip transe_emit_rounds_body: rounds of one corruption
kind, raw buffer gathers, one merged reduction per round -- engine option emit_rounds = 1, the default) against the body it
replaces (transe_emit_vec_v1_kernel, emit_rounds = 0) on identical inputs.

Both sum the same floats in the same association (csrc/team.hpp team_sum4 forms, lane by lane, the sums team_sum<64> forms) and
the same integer signs, so everything the kernel writes must be equal BIT FOR BIT: destination keys, int8 records, 2-bit
records, the loss, and -- after one Adam step through Config.train_step -- the tables and both moments.  No tolerance anywhere.
The arithmetic itself is checked against the oracle by test_gpu_models.py / test_gpu_configs.py, which run the new body.

Shapes: D = 132 / 200 / 256 leave 33 / 50 / 64 live lanes of the 64; n = 1, 3, 4, 5, 25, 63 negatives give a remainder round
of every size, full rounds only, and the most the count path takes; B = 37 leaves idle waves in the last workgroup.  n = 70
(a second round of ids) is refused by every entry point of the sign-count path (1..63 negatives: int8 sums), so that case
asserts the refusal, which does not depend on the option."""
import ctypes

import numpy as np
import pytest

from test_gpu_models import make_engine

pytestmark = pytest.mark.gpu

E, R, B = 97, 7, 37
DIMS = [132, 200, 256]
NEGS = [1, 3, 4, 5, 25, 63, 70]
KINDS = ["head", "tail", "mixed", "mixed_rel"]
MARGIN = 0.5          # random rows: p - score spreads about +-1 around 0, so a good part of the hinges falls on either side


def tables(D, seed):
    """Random tables with whole columns of exact +-0 (test_gpu_models.py::test_negative_zero_has_sign_zero): e = h^ + r^ - t^ and
    fma(f, x, B) are exactly -0.0 / +0.0 there, in the first lanes and in the last live one."""
    rng = np.random.default_rng(seed)
    ent = rng.standard_normal((E, D)).astype(np.float32)
    rel = rng.standard_normal((R, D)).astype(np.float32)
    ent[0::2, 0] = -0.0; ent[1::2, 0] = 0.0; rel[:, 0] = -0.0
    ent[:, 1] = 0.0; rel[:, 1] = 0.0
    ent[:, 2] = -0.0; rel[:, 2] = 0.0
    ent[:, 3] = -0.0; rel[:, 3] = -0.0
    ent[:, D - 1] = -0.0; rel[:, D - 1] = -0.0
    ent[:, 5] = 0.0; rel[0::2, 5] = -0.0; rel[1::2, 5] = 0.0
    return ent, rel


def batch(rng, n, kind, deferred_group=None):
    """[3, B * (1 + n)] ids, slot of negative k of group b at b + (k + 1) * B; every negative differs from its positive in exactly
    one slot, except negative n // 2 of `deferred_group`, which differs in two."""
    h = rng.integers(0, E, B); t = rng.integers(0, E, B); r = rng.integers(0, R, B)
    H, T, Rr = [h], [t], [r]
    for k in range(n):
        which = {"head": np.zeros(B, int), "tail": np.ones(B, int), "mixed": rng.integers(0, 2, B),
                 "mixed_rel": rng.integers(0, 3, B)}[kind]
        nh = np.where(which == 0, (h + 1 + rng.integers(0, E - 1, B)) % E, h)
        nt = np.where(which == 1, (t + 1 + rng.integers(0, E - 1, B)) % E, t)
        nr = np.where(which == 2, (r + 1 + rng.integers(0, R - 1, B)) % R, r)
        if deferred_group is not None and k == n // 2:
            nh[deferred_group] = (h[deferred_group] + 1) % E; nt[deferred_group] = (t[deferred_group] + 2) % E
        H.append(nh); T.append(nt); Rr.append(nr)
    return np.stack([np.concatenate(H), np.concatenate(T), np.concatenate(Rr)]).astype(np.int32)


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    L.kge_set_option(b"emit_rounds", 1)
    L.kge_set_option(b"inv_table_max_bytes", 256 << 20)


def desc_for(D, nr):
    from openkeonspark_amd import _lib
    d = _lib.ModelDesc()
    d.model = 0; d.negative_rel = nr; d.ent_total = E; d.rel_total = R; d.ent_dim = D; d.rel_dim = D; d.margin = MARGIN
    return d


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def run_emit(L, rounds, desc, ent, rel, ids, n, with_resid):
    """kge_transe_emit_records into zeroed buffers -> (rc, dst, rec, loss, deferred groups, residuals)."""
    import torch
    L.kge_set_option(b"emit_rounds", rounds)
    L.kge_set_option(b"tables_changed", 0)
    M = B * (3 + n)
    dw = int(L.kge_transe_record_dwords(ctypes.byref(desc)))
    rec = torch.zeros((M, dw), dtype=torch.int32, device="cuda")
    dst = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    ge = torch.zeros_like(ent); gr = torch.zeros_like(rel)
    rc = L.kge_transe_emit_records(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), ids[0].data_ptr(), ids[1].data_ptr(),
                                   ids[2].data_ptr(), B, n, B, B, rec.data_ptr(), dst.data_ptr(),
                                   ge.data_ptr() if with_resid else None, gr.data_ptr() if with_resid else None, loss.data_ptr(), None)
    nd = ctypes.c_int32(-1)
    if rc == 0:
        assert L.kge_transe_deferred_groups(ctypes.byref(nd)) == 0
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy(), rec.cpu().numpy(), loss.cpu().numpy(), nd.value, ge.cpu().numpy(), gr.cpu().numpy()


@pytest.mark.parametrize("inv_table", [True, False])
@pytest.mark.parametrize("D", DIMS)
def test_emit_records_equal_bit_for_bit(lib, D, inv_table):
    """kge_transe_emit_records, every n and corruption mix, with the per-row 1/|row| table and with the norms taken from the
    gathered rows; the "mixed" batches carry one group that must be deferred (listed, all its keys -1) exactly as before."""
    import torch
    lib.kge_set_option(b"inv_table_max_bytes", (256 << 20) if inv_table else 0)
    ent_h, rel_h = tables(D, D)
    ent = torch.from_numpy(ent_h).cuda(); rel = torch.from_numpy(rel_h).cuda()
    rng = np.random.default_rng(1000 + D)
    seen_active = seen_idle = 0
    for n in NEGS:
        for kind in KINDS:
            g = 11 if kind == "mixed" else None
            desc = desc_for(D, 1 if kind == "mixed_rel" else 0)
            ids = torch.from_numpy(batch(rng, n, kind, g)).cuda()
            old = run_emit(lib, 0, desc, ent, rel, ids, n, with_resid=(kind == "tail"))
            new = run_emit(lib, 1, desc, ent, rel, ids, n, with_resid=(kind == "tail"))
            if n > 63:
                assert old[0] != 0 and new[0] == old[0], (n, old[0], new[0])
                continue
            assert old[0] == 0 and new[0] == 0
            what = (D, inv_table, n, kind)
            assert np.array_equal(old[1], new[1]), ("dst",) + what
            assert np.array_equal(old[2], new[2]), ("int8 records",) + what
            assert np.array_equal(bits(old[3]), bits(new[3])), ("loss", float(old[3][0]), float(new[3][0])) + what
            assert old[4] == new[4] == (1 if g is not None else 0), ("deferred",) + what
            assert np.array_equal(bits(old[5]), bits(new[5])) and np.array_equal(bits(old[6]), bits(new[6])), ("residuals",) + what
            dst = new[1].reshape(3 + n, B)
            assert not (dst == -7).any()                       # every key was written
            if g is not None:
                assert (dst[:, g] == -1).all()
            live = np.ones(B, bool)
            if g is not None:
                live[g] = False
            neg = dst[3:, live]
            seen_active += int((neg >= 0).sum()); seen_idle += int((neg < 0).sum())
            if kind == "mixed_rel" and n >= 25:
                assert (neg >= E).any()                        # relation-vector corruptions (code 2) with an active hinge
            if kind in ("head", "tail") and n >= 4:
                assert (neg >= 0).any() and (neg < 0).any(), what
    assert seen_active > 0 and seen_idle > 0
    assert min(seen_active, seen_idle) > 0.05 * (seen_active + seen_idle), (seen_active, seen_idle)


def run_counts(L, rounds, desc, ent, rel, ids, n):
    import torch
    L.kge_set_option(b"emit_rounds", rounds)
    L.kge_set_option(b"tables_changed", 0)
    counts = torch.zeros((E + R, desc.ent_dim), dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    ge = torch.zeros_like(ent); gr = torch.zeros_like(rel)
    rc = L.kge_transe_forward_counts(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), ids[0].data_ptr(), ids[1].data_ptr(),
                                     ids[2].data_ptr(), B, n, B, B, counts.data_ptr(), ge.data_ptr(), gr.data_ptr(), loss.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy(), loss.cpu().numpy(), ge.cpu().numpy(), gr.cpu().numpy()


@pytest.mark.parametrize("inv_table", [True, False])
@pytest.mark.parametrize("D", DIMS)
def test_forward_counts_equal_bit_for_bit(lib, D, inv_table):
    """kge_transe_forward_counts: the summed int32 counts, the loss and the fp32 residuals of the deferred group."""
    import torch
    lib.kge_set_option(b"inv_table_max_bytes", (256 << 20) if inv_table else 0)
    ent_h, rel_h = tables(D, 7 * D)
    ent = torch.from_numpy(ent_h).cuda(); rel = torch.from_numpy(rel_h).cuda()
    rng = np.random.default_rng(2000 + D)
    resid_seen = False
    for n in NEGS:
        for kind in KINDS:
            desc = desc_for(D, 1 if kind == "mixed_rel" else 0)
            ids = torch.from_numpy(batch(rng, n, kind, 5 if kind == "mixed" else None)).cuda()
            old = run_counts(lib, 0, desc, ent, rel, ids, n)
            new = run_counts(lib, 1, desc, ent, rel, ids, n)
            if n > 63:
                assert old[0] != 0 and new[0] == old[0]
                continue
            assert old[0] == 0 and new[0] == 0
            what = (D, inv_table, n, kind)
            assert old[1].any(), what
            assert np.array_equal(old[1], new[1]), ("counts",) + what
            assert np.array_equal(bits(old[2]), bits(new[2])), ("loss", float(old[2][0]), float(new[2][0])) + what
            assert np.array_equal(bits(old[3]), bits(new[3])) and np.array_equal(bits(old[4]), bits(new[4])), ("residuals",) + what
            resid_seen = resid_seen or bool(old[3].any())
    assert resid_seen                                          # the deferred groups went through the exact fp32 pass


def adam_step(L, rounds, D, n, nr, params, ids):
    """One fused TF1-Adam step (2-bit negative records) on a hand-made batch -> loss, tables, moments, the step's keys and records."""
    import torch
    L.kge_set_option(b"emit_rounds", rounds)
    con = make_engine("transe", E, R, D, n - nr, nr, margin=MARGIN, opt="Adam", alpha=0.001, params=params)
    assert con.use_counts and getattr(con, "fused_counts", True) and con._adam and not con.sparse_rows
    h, t, r = (ids[i].astype(np.int64) for i in range(3))
    loss = con.train_step(h, t, r, None)
    torch.cuda.synchronize()
    out = {k: v.copy() for k, v in con.get_parameters().items()}
    for i, k in enumerate(con.trainModel.table_names):
        out["m/" + k] = con._adam_m[i].cpu().numpy()
        out["v/" + k] = con._adam_v[i].cpu().numpy()
    M, dw = B * (3 + n), int(L.kge_transe_record_dwords(ctypes.byref(con._desc)))
    keys = np.zeros(M, np.int32)
    assert L.kge_transe_step_scratch_read(1, 0, M, keys.ctypes.data) == 0
    rec8 = np.zeros((3 * B, dw), np.uint32)
    assert L.kge_transe_step_scratch_read(0, 0, rec8.size, rec8.ctypes.data) == 0
    rec2 = np.zeros((n * B, dw), np.uint8)                    # dw bytes per 2-bit record: one per lane
    assert L.kge_transe_step_scratch_read(0, rec8.size, rec2.size // 4, rec2.ctypes.data) == 0
    return loss, out, keys, rec8, rec2


@pytest.mark.parametrize("n,nr", [(3, 0), (25, 5), (63, 9)])
@pytest.mark.parametrize("D", DIMS)
def test_adam_step_and_two_bit_records_equal_bit_for_bit(lib, D, n, nr):
    """Config.train_step with the fused count step: keys, the positives' int8 records, the negatives' 2-bit records (live lanes
    of the records with an active hinge: the others are never written), loss, tables and Adam moments."""
    ent_h, rel_h = tables(D, 13 * D + n)
    params = {"ent_embeddings": ent_h, "rel_embeddings": rel_h}
    ids = batch(np.random.default_rng(3000 + D + n), n, "mixed_rel" if nr else "mixed", None)
    lo, so, ko, r8o, r2o = adam_step(lib, 0, D, n, nr, params, ids)
    ln, sn, kn, r8n, r2n = adam_step(lib, 1, D, n, nr, params, ids)
    assert np.float32(lo).tobytes() == np.float32(ln).tobytes(), (lo, ln)
    assert np.array_equal(ko, kn)
    live = (ko >= 0) & (ko < 2 * (E + R))                                    # keys are 2 * row + kind; anything else: no record
    pos_live, neg_live = live[:3 * B], live[3 * B:]
    assert neg_live.any() and not neg_live.all()                             # active and idle hinges
    assert (ko[3 * B:][neg_live] % 2 == 1).all() and (ko[:3 * B][pos_live] % 2 == 0).all()
    assert np.array_equal(r8o[pos_live], r8n[pos_live])
    assert np.array_equal(r2o[neg_live][:, :D // 4], r2n[neg_live][:, :D // 4])
    assert r2n[neg_live][:, :D // 4].any()
    for k in so:
        assert np.array_equal(bits(so[k]), bits(sn[k])), k
    assert not np.array_equal(so["ent_embeddings"], ent_h)                   # the step moved the table
