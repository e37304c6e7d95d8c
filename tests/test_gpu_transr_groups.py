"""TransR's group layout (csrc/transr.hip GemmArgs: groups of one positive and its n negatives sorted by relation, a group's
U = 2 + n rows side by side in a 16-row sub-tile, the rest of the sub-tile pad rows; the vector stage in the projection's
epilogue) against the fp64 autograd restatement of the reference graph (tests/torch_ref.py, TransR.py:16-75).

Batches are built by hand to the kge_forward_backward_sampled contract (include/kge_mi355.h: every negative differs from its
positive in exactly one entity) and laid out with a stride larger than the positive count, the gaps filled with ids that would
change the result if they were read.  Every run asserts that the layout was taken (kge_transr_group_layout_active) and that
every row the batch does not touch has a gradient of exactly zero.  Entity 0 -- the entity of the pad rows -- has a normal
row and is kept out of the batches except where noted, so a pad row that leaks into dgrad shows up there.

The matrix: every (De, Dr) below with n = 1, 5, 14 (gps = 16 / U = 5, 2, 1 groups per sub-tile); the full n sweep at one
wgrad_kernel shape and one wgrad3_kernel shape; the separate vector stage (lean and generic) and dgrad's float records at a
few shapes; relation buckets at their edges (one relation, R = 1023 where the relation histogram is exactly full, relations
of exactly gps, gps + 1 and 8 gps groups, R = 1024 where the layout is not taken).  The sequence tests replay the call orders
that left a stale pad row behind (a GP row of another call in the pad slot's place)."""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest

from oracle import oracle
from test_gpu_models import RTOL, batch_without_ties, check_gradients_with_kinks, make_engine, seed_of

pytestmark = pytest.mark.gpu

DEFAULTS = {"transr_groups": 1, "transr_fuse_vec": 1, "transr_lean": 1, "transr_dgrad_records": 1, "transr_dgrad_records_min": 1 << 15}
VARIANTS = {
    "fused": {},
    "separate-lean": {"transr_fuse_vec": 0},
    "separate-generic": {"transr_fuse_vec": 0, "transr_lean": 0},
    "dgrad-records": {"transr_dgrad_records_min": 0},
}
Z, T = 1, 2          # entity rows of zeros / with a squared norm below 1e-12 (normalise's clamped branch)
N_GAP = 6            # the last N_GAP entities appear only in the stride gaps
GAP = 37             # stride = n_pos + GAP

# (De, Dr): rows_gemm3<PROJECT, 7 | 13> (Dr <= 112 | above) x rows_gemm3<DGRAD, 7 | 13> (De <= 112 | above), heavy column
# padding (Dr = 8, 16, 100, 116), wgrad_kernel (De <= 192 or Dr <= 192) against wgrad3_kernel (both > 192)
SHAPES = [(12, 8), (64, 100), (100, 116), (116, 112), (208, 16), (192, 196), (196, 196), (208, 208), (200, 200)]


@contextmanager
def options(**kw):
    from openkeonspark_amd import _lib
    L = _lib.lib()
    try:
        L.kge_set_option(b"transr_groups", 2)          # the layout at any batch size
        for k, v in kw.items():
            L.kge_set_option(k.encode(), v)
        yield L
    finally:
        for k, v in DEFAULTS.items():
            L.kge_set_option(k.encode(), v)


def make_params(E, R, De, Dr, seed, r_zero=None):
    params = oracle.init_params(oracle.TRANSR, E, R, De, Dr, seed=seed)
    for k in params:
        params[k] = (params[k] * 3).astype(np.float32)
    params["ent_embeddings"][Z] = 0.0
    params["ent_embeddings"][T] *= np.float32(1e-9)
    if r_zero is not None:
        params["rel_embeddings"][r_zero] = 0.0
    return params


def make_groups(rng, E, rels, n, ent0=False):
    """Compact batch (positives, then negative k of every positive): positives of the given relations, each negative a
    single-entity corruption -- both sides, the positive's other entity (h' = t, t' = h), one hot entity across groups, the
    previous negative's new entity again, the zero and the tiny row; 5 % self-loop positives."""
    B = len(rels)
    lo, hi = (0 if ent0 else 1), E - N_GAP
    h = rng.integers(lo, hi, B)
    t = rng.integers(lo, hi, B)
    loops = rng.random(B) < 0.05
    t[loops] = h[loops]
    h[rng.integers(0, B, 3)] = Z
    t[rng.integers(0, B, 3)] = T
    hot = int(rng.integers(lo, hi))
    H, Tt = [h], [t]
    prev = None
    for k in range(n):
        side = rng.random(B) < 0.5                    # True: a new head
        old = np.where(side, h, t)
        other = np.where(side, t, h)
        new = rng.integers(lo, hi, B)
        pick = rng.random(B)
        new = np.where(pick < 0.1, other, new)
        new = np.where((pick >= 0.1) & (pick < 0.2), hot, new)
        new = np.where((pick >= 0.2) & (pick < 0.23), Z, new)
        new = np.where((pick >= 0.23) & (pick < 0.26), T, new)
        if prev is not None:
            new = np.where((pick >= 0.26) & (pick < 0.36), prev, new)
        clash = new == old
        new[clash] = lo + (old[clash] - lo + 1 + rng.integers(0, hi - lo - 1, int(clash.sum()))) % (hi - lo)
        H.append(np.where(side, new, h))
        Tt.append(np.where(side, t, new))
        prev = new
    return np.concatenate(H), np.concatenate(Tt), np.tile(np.asarray(rels, np.int64), n + 1)


def strided(rng, E, bh, bt, br, B, n, r_gap):
    """[3, n_pos + n * stride] int32 with stride = B + GAP: block k at k * stride, the gaps entities and a relation no live
    position has."""
    stride = B + GAP
    L = B + n * stride
    out = np.empty((3, L), np.int64)
    out[0] = rng.integers(E - N_GAP, E, L)
    out[1] = rng.integers(E - N_GAP, E, L)
    out[2] = r_gap
    for k in range(n + 1):
        out[:, k * stride:k * stride + B] = np.stack([bh, bt, br])[:, k * B:(k + 1) * B]
    return out.astype(np.int32), stride


def run_engine(con, L, lay, B, n, stride, denom, sampler_shaped=True):
    import torch
    dev = torch.from_numpy(lay).cuda()
    for g in con._grads:
        g.zero_()
    con.forward_backward(dev, B, stride, denom, sampler_shaped=sampler_shaped)
    torch.cuda.synchronize()
    return float(con._loss.item()), con.get_gradients()


def layout_active(L, con, B, n):
    return L.kge_transr_group_layout_active(ctypes.byref(con._desc), B, n)


def check_against_fp64(params, bh, bt, br, B, n, De, Dr, margin, denom, loss_g, g_g, special):
    """Loss within 1e-5 relative, every gradient table within RTOL of fp64 (kink rows as in test_gpu_models), untouched rows
    exactly 0.  `special`: {table: rows} of zero / tiny rows whose gradient carries 1 / sqrt(1e-12) -- compared on their own
    scale, and out of the table-wide comparison whose scale they would swamp."""
    from torch_ref import loss_and_grads, near_kink_rows
    loss_r, g_r = loss_and_grads("transr", params, bh, bt, br, B, n, margin, De, Dr)
    s = B * n / denom                                    # the reference is a mean over B n hinges
    loss_r *= s
    g_r = {k: v * s for k, v in g_r.items()}
    assert abs(loss_g - loss_r) <= RTOL * abs(loss_r), (loss_g, loss_r)
    # rows the batch does not reach: exactly zero (matrices: the positives' relations only, negative_rel == 0)
    live = {"ent_embeddings": set(bh.tolist()) | set(bt.tolist()), "rel_embeddings": set(br.tolist()),
            "transfer_matrix": set(br[:B].tolist())}
    for k, rows in live.items():
        dead = np.setdiff1d(np.arange(g_g[k].shape[0]), np.fromiter(rows, np.int64))
        nz = dead[(g_g[k][dead] != 0).any(1)]
        assert nz.size == 0, (k, "nonzero gradient on rows the batch does not touch", nz[:8].tolist())
    gg = {k: v.astype(np.float64).copy() for k, v in g_g.items()}
    gr = {k: v.copy() for k, v in g_r.items()}
    kink = None
    for k, rows in special.items():
        for row in rows:
            if row not in live[k]:
                continue
            err = np.abs(gg[k][row] - gr[k][row]).max()
            if err > RTOL * (np.abs(gr[k][row]).max() + 1e-30):
                if kink is None:
                    kink, _ = near_kink_rows("transr", params, bh, bt, br, B, n, De, Dr, tol=1e-7)
                assert row in kink[k], (k, row, err, np.abs(gr[k][row]).max())
            gg[k][row] = 0.0
            gr[k][row] = 0.0
    check_gradients_with_kinks("transr", params, bh, bt, br, B, n, (De, Dr), 0, None, gg, gr)


def run_case(E, R, De, Dr, n, rels, variant="fused", margin=1.0, seed=0, ent0=False, r_zero=0, r_gap=None, expect_layout=1):
    rng = np.random.default_rng(seed)
    params = make_params(E, R, De, Dr, seed % 1000, r_zero)
    orc = oracle.Model("transr", E, R, De, Dr, margin=margin, params=params)
    B = len(rels)
    bh, bt, br = batch_without_ties(orc, lambda: make_groups(rng, E, rels, n, ent0), B, n)
    lay, stride = strided(rng, E, bh, bt, br, B, n, R - 1 if r_gap is None else r_gap)
    denom = B * n + 7
    with options(**VARIANTS[variant]) as L:
        con = make_engine("transr", E, R, De, n, 0, margin=margin, params=params, Dr=Dr)
        assert layout_active(L, con, B, n) == expect_layout
        loss_g, g_g = run_engine(con, L, lay, B, n, stride, denom)
    special = {"ent_embeddings": [Z, T], "rel_embeddings": [] if r_zero is None else [r_zero]}
    check_against_fp64(params, bh, bt, br, B, n, De, Dr, margin, denom, loss_g, g_g, special)


def uniform_rels(rng, B, R_live, r_zero=0):
    rels = rng.integers(0, R_live, B)
    rels[0] = r_zero
    return rels


@pytest.mark.parametrize("De,Dr", SHAPES)
@pytest.mark.parametrize("n", [1, 5, 14])
def test_group_layout_shapes(De, Dr, n):
    """Eleven relations (the last only in the stride gaps), B = 300: 27 groups per relation, several sub-tiles each (at n = 1
    the fifth group of a full sub-tile takes the epilogue's second team pass); wgrad3 shapes take span 1 at n = 1 and 5 and
    SPAN2 at n = 14 (rows_max against 256 R)."""
    E, R, B = 300, 12, 300
    rng = np.random.default_rng(seed_of("groups-rels", De, Dr, n))
    run_case(E, R, De, Dr, n, uniform_rels(rng, B, R - 1), seed=seed_of("groups", De, Dr, n))


@pytest.mark.parametrize("De,Dr", [(100, 116), (200, 200)])
@pytest.mark.parametrize("n", [2, 3, 4, 6, 7, 10])
def test_group_layout_negative_counts(De, Dr, n):
    """U = 4 .. 12: gps 4, 3, 2, 2, 1, 1 and 0 .. 8 pad rows per sub-tile, on wgrad_kernel and on wgrad3_kernel."""
    E, R, B = 300, 8, 260
    rng = np.random.default_rng(seed_of("nsweep-rels", De, Dr, n))
    run_case(E, R, De, Dr, n, uniform_rels(rng, B, R - 1), seed=seed_of("nsweep", De, Dr, n))


@pytest.mark.parametrize("variant", ["separate-lean", "separate-generic", "dgrad-records"])
@pytest.mark.parametrize("De,Dr,n", [(12, 8, 5), (116, 112, 1), (208, 208, 3)])
def test_group_layout_variants(variant, De, Dr, n):
    """The vector stage as its own launch on P (the lean kernel; the generic one behind a memset of GP) and dgrad's rows as
    float records with a segmented sum, at a slot count far below the records' default threshold."""
    E, R, B = 300, 10, 280
    rng = np.random.default_rng(seed_of("variant-rels", De, Dr, n))
    run_case(E, R, De, Dr, n, uniform_rels(rng, B, R - 1), variant=variant, seed=seed_of("variant", variant, De, Dr, n))


def skewed_rels(rng, gps, R):
    sizes = [gps, gps + 1, 8 * gps, 1, 2 * gps + 1, 3]
    rels = np.concatenate([np.full(s, r) for r, s in enumerate(sizes)] + [rng.integers(len(sizes), R - 1, 60)])
    return rng.permutation(rels)


BUCKETS = [("one-relation", 64, 100), ("one-relation", 208, 208), ("skewed", 64, 100), ("skewed", 208, 208), ("r1023", 64, 100),
           ("r1024", 64, 100)]


@pytest.mark.parametrize("bucket,De,Dr", BUCKETS)
@pytest.mark.parametrize("n", [1, 6])
def test_group_layout_buckets(bucket, De, Dr, n):
    """one-relation: R = 1 (entity 0 inside the batch, no zero relation row) over several 128-row tiles -- wgrad3's 512-row
    spans; skewed: relations of exactly gps, gps + 1 and 8 gps groups next to one-group relations; r1023: (R + 1) * 4 fills
    the relation histogram exactly, most relations empty; r1024: one relation more, the layout is not taken and the same
    sampler-shaped call goes through the radix-sorted three-kernel path."""
    rng = np.random.default_rng(seed_of("bucket-rels", bucket, De, Dr, n))
    gps = 16 // (2 + n)
    seed = seed_of("bucket", bucket, De, Dr, n)
    if bucket == "one-relation":
        run_case(260, 1, De, Dr, n, np.zeros(400 if n == 1 else 200, np.int64), seed=seed, ent0=True, r_zero=None, r_gap=0)
    elif bucket == "skewed":
        run_case(300, 12, De, Dr, n, skewed_rels(rng, gps, 12), seed=seed)
    else:
        R = 1023 if bucket == "r1023" else 1024
        used = np.concatenate([[0, R - 2], rng.choice(np.arange(1, R - 2), 22, replace=False)])
        rels = used[rng.integers(0, len(used), 300)]
        rels[0] = 0
        run_case(300, R, De, Dr, n, rels, seed=seed, expect_layout=1 if R == 1023 else 0)


# ---- call sequences that left a stale pad row: a margin above any score difference (3 sqrt(Dr) at most) makes every hinge
# active, so every GP row a call writes is nonzero ----
ALL_ON = 64.0


def all_active_batch(rng, orc, E, rels, n):
    B = len(rels)
    bh, bt, br = make_groups(rng, E, rels, n)
    assert (orc.hinge_margins(bh, bt, br, B, n) > 0).all()
    return bh, bt, br


@pytest.mark.parametrize("first,second", [((64, 96), (64, 48)), ((208, 208), (196, 196))])
@pytest.mark.parametrize("variant", ["fused", "separate-lean"])
def test_second_config_with_narrower_rel_dim(first, second, variant):
    """Two Configs in one process, same E, R, B and n, the second with the smaller Dr: its pad slot's GP row (GP + slots Dr)
    lies inside the GP rows the first call wrote.  The second Config's gradients must not see them (wgrad_kernel for the
    first pair, wgrad3_kernel for the second)."""
    E, R, B, n = 300, 6, 300, 1
    rng = np.random.default_rng(seed_of("second-config", first, second, variant))
    rels = uniform_rels(rng, B, R - 1)
    with options(**VARIANTS[variant]) as L:
        for i, (De, Dr) in enumerate((first, second)):
            params = make_params(E, R, De, Dr, seed=20 + i)
            orc = oracle.Model("transr", E, R, De, Dr, margin=ALL_ON, params=params)
            bh, bt, br = all_active_batch(rng, orc, E, rels, n)
            bh[B], bt[B] = (bh[0] + 1) % (E - N_GAP) or 1, bt[0]      # positive 0's first negative: a new head (canonical slot 2 B)
            lay, stride = strided(rng, E, bh, bt, br, B, n, R - 1)
            con = make_engine("transr", E, R, De, n, 0, margin=ALL_ON, params=params, Dr=Dr)
            assert layout_active(L, con, B, n) == 1
            loss_g, g_g = run_engine(con, L, lay, B, n, stride, B * n + 7)
    check_against_fp64(params, bh, bt, br, B, n, De, Dr, ALL_ON, B * n + 7, loss_g, g_g, {"ent_embeddings": [Z, T], "rel_embeddings": [0]})


@pytest.mark.parametrize("De,Dr", [(64, 96), (208, 208)])
def test_group_call_after_larger_three_kernel_call(De, Dr):
    """One Config: a large call (the workspace is not regrown after it), a group-layout call at B1, a three-kernel call at
    B2 > B1 (1 + n) -- its prep and lean vector stage write job_ent and the GP row of slot 2 B1 (1 + n), the group layout's pad
    slot at B1 -- and the group-layout call at B1 again, which must match fp64."""
    E, R, n = 300, 6, 1
    B0, B1 = 1200, 200
    B2 = B1 * (1 + n) + 50
    rng = np.random.default_rng(seed_of("after-three-kernel", De, Dr))
    params = make_params(E, R, De, Dr, seed=30)
    orc = oracle.Model("transr", E, R, De, Dr, margin=ALL_ON, params=params)
    with options() as L:
        con = make_engine("transr", E, R, De, n, 0, margin=ALL_ON, params=params, Dr=Dr)
        batches = {}
        for B in (B0, B1, B2):
            bh, bt, br = all_active_batch(rng, orc, E, uniform_rels(rng, B, R - 1), n)
            batches[B] = (bh, bt, br) + strided(rng, E, bh, bt, br, B, n, R - 1)
        for B, shaped in ((B0, True), (B1, True), (B2, False), (B1, True)):
            bh, bt, br, lay, stride = batches[B]
            assert layout_active(L, con, B, n) == 1      # (the query is about sampler-shaped calls: the B2 call is not one)
            loss_g, g_g = run_engine(con, L, lay, B, n, stride, B * n + 7, sampler_shaped=shaped)
    bh, bt, br = batches[B1][:3]
    check_against_fp64(params, bh, bt, br, B1, n, De, Dr, ALL_ON, B1 * n + 7, loss_g, g_g, {"ent_embeddings": [Z, T], "rel_embeddings": [0]})
