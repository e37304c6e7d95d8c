"""Shapes and batches of tests/test_gpu_size_gates.py: the smallest steps that cross the engine's size gates -- relation-row
copies of the TransE sign-count path (from 4096 groups), the chunk lengths of the float-record segmented sum (2^18 and 2^20
records), the second trip of the grid-capped emit / forward-backward kernels (more than 4096 * 16 groups for 16-lane teams).

Everything here runs on the CPU; tests/test_size_gate_cases.py builds every case without a GPU and checks, through the engine's
host-only queries, that the case crosses its gate.  The batches are cached, so the GPU tests that share a case build it once."""
import functools

import numpy as np

from oracle import oracle
from test_gpu_models import rand_batch, seed_of

MAX_REDRAW_SHARE = 0.05      # of the groups, over all rounds
HINGE_TIE = 1e-4             # batch_without_ties' distance of a hinge from its switch point
KINK = 1e-6                  # an element of e = h^ + r^ - t^ this close to zero (fp64) may take either sign in fp32

RECORD_SLOTS = {"transe": lambda n: 3 + n, "transh": lambda n: 4 + n, "transd": lambda n: 6 + 2 * n}   # csrc/models.hip record_space


def transe_kink_groups(params, bh, bt, br, B, N):
    """Groups with an element of e within KINK of zero, e in fp64 from the fp32 tables (as torch_ref.near_kink_rows forms it)."""
    l2 = lambda x: x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12))
    en, rn = l2(params["ent_embeddings"].astype(np.float64)), l2(params["rel_embeddings"].astype(np.float64))
    near = np.zeros(B * (1 + N), bool)
    step = max(1, (1 << 22) // en.shape[1])
    for lo in range(0, len(near), step):
        s = slice(lo, lo + step)
        near[s] = (np.abs(en[bh[s]] + rn[br[s]] - en[bt[s]]) < KINK).any(-1)
    return np.unique(np.nonzero(near)[0] % B)


def batch_without_ties_by_group(orc, rng, E, R, B, n, nr, foreign=0.0, distinct=False, kinks=False):
    """rand_batch, then only the groups with a hinge within HINGE_TIE of zero (kinks=True, TransE: or an element of e within KINK
    of zero) drawn again, until none is left.  Returns (bh, bt, br), share of the groups redrawn over all rounds (asserted to
    stay within MAX_REDRAW_SHARE: a case over it gets another seed or margin, not another cap)."""
    N = n + nr
    h, t, r = rand_batch(rng, E, R, B, n, nr, foreign, distinct)
    slots = B * np.arange(1 + N)[:, None]
    redrawn = 0
    for _ in range(100):
        bad = np.nonzero((np.abs(orc.hinge_margins(h, t, r, B, N)) <= HINGE_TIE).any(1))[0]
        if kinks:
            bad = np.union1d(bad, transe_kink_groups(orc.params, h, t, r, B, N))
        if not len(bad):
            return (h, t, r), redrawn / B
        redrawn += len(bad)
        assert redrawn <= MAX_REDRAW_SHARE * B, ("redrew %d of %d groups" % (redrawn, B))
        idx = (slots + bad[None, :]).ravel()          # slot-major, the layout of a batch of len(bad) groups
        h[idx], t[idx], r[idx] = rand_batch(rng, E, R, len(bad), n, nr, foreign, distinct)
    raise AssertionError("no tie-free batch found")


def check_layout(bh, bt, br, B, n, nr, E, R, sampler_shaped):
    """The reference's flat batch (Base.cpp:109-139): slot k of group b at B k + b, ids in range; sampler_shaped: every entity
    negative keeps the relation and changes exactly one entity, every relation negative changes the relation alone."""
    N = n + nr
    assert len(bh) == len(bt) == len(br) == B * (1 + N)
    assert bh.min() >= 0 and bt.min() >= 0 and br.min() >= 0 and bh.max() < E and bt.max() < E and br.max() < R
    if not sampler_shaped:
        return
    h, t, r = (x.reshape(1 + N, B) for x in (bh, bt, br))
    assert (r[1:1 + n] == r[:1]).all() and ((h[1:1 + n] == h[:1]) ^ (t[1:1 + n] == t[:1])).all()
    assert (h[1 + n:] == h[:1]).all() and (t[1 + n:] == t[:1]).all() and (r[1 + n:] != r[:1]).all()


def numpy_sign_counts(params, bh, bt, br, B, N, margin):
    """test_gpu_models.numpy_sign_counts with the loop over the groups replaced by np.add.at: the integer sign-count gradient
    of the TransE loss w.r.t. the NORMALISED rows (TransE.py:11-15,48-51), rows [0,E) entities, [E,E+R) relations."""
    ent, rel = params["ent_embeddings"], params["rel_embeddings"]
    E, D = ent.shape
    l2 = lambda x: x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12)).astype(np.float32)
    en, rn = l2(ent), l2(rel)
    S = np.zeros((E + rel.shape[0], D), np.int64)
    e_p = en[bh[:B]] + rn[br[:B]] - en[bt[:B]]
    p = np.abs(e_p).sum(-1)
    sp = np.sign(e_p).astype(np.int64)
    for k in range(N):
        sl = slice(B * (k + 1), B * (k + 2))
        e_k = en[bh[sl]] + rn[br[sl]] - en[bt[sl]]
        a = np.nonzero((p - np.abs(e_k).sum(-1) + np.float32(margin)) >= 0)[0]
        sk = np.sign(e_k).astype(np.int64)
        np.add.at(S, bh[a], sp[a]); np.add.at(S, E + br[a], sp[a]); np.subtract.at(S, bt[a], sp[a])
        np.subtract.at(S, bh[sl][a], sk[a]); np.subtract.at(S, E + br[sl][a], sk[a]); np.add.at(S, bt[sl][a], sk[a])
    return S


def oracle_grad(orc, bh, bt, br, B, N, groups=32):
    """(loss, {table: dL/dtable, fp64}) of the oracle with the ROWS' sums taken in fp64: the oracle's gradient of every `groups`
    consecutive groups (denominator B N), added in double.  orc.grad adds a row's contributions one by one in fp32, which is
    exact enough for a few hundred of them; the relation rows of these cases collect 10^4 - 10^5 each, where that sequential
    sum is itself off by 6e-5 - 2e-4 of the table's largest element (measured against this form at 2^18 and 2^20 records; the
    entity rows by < 1e-6) -- more than the 1e-5 the kernels are held to.  The form converges: 32 and 64 groups per slice agree
    to ~1e-6 on those cases (tests/test_size_gate_cases.py checks it on one)."""
    loss, full = orc.grad(bh, bt, br, B, N)
    acc = {k: np.zeros(v.shape, np.float64) for k, v in full.items()}
    slots = B * np.arange(1 + N)[:, None]
    for lo in range(0, B, groups):
        hi = min(B, lo + groups)
        idx = (slots + np.arange(lo, hi)[None, :]).ravel()
        g = orc.grad(bh[idx], bt[idx], br[idx], hi - lo, N, denom=B * N)[1]
        for k in g:
            acc[k] += g[k]
    return loss, acc


def scaled_params(model, E, R, D, seed, Dr=None):
    params = oracle.init_params(oracle.MODEL_IDS[model], E, R, D, D if Dr is None else Dr, seed=seed)
    return {k: (v * 3).astype(np.float32) for k, v in params.items()}


# ---- C1: relation-row copies of the sign-count path ---------------------------------------------------------------------------
COUNT_DN = [(16, 3), (64, 1), (100, 2), (7, 3), (50, 1), (200, 1)]      # team shapes 16x4, 32x4, 64x4; D % 4 != 0: scalar emit, non-natural records
# (E, R, D, n, B, option counts_krel, copies the engine must report)
EXACT_CASES = [(61, 4, D, n, B, 4, 4 if B >= 4096 else 1) for D, n in COUNT_DN for B in (4095, 4096, 4097)] \
    + [(10, 40, D, n, 4096, 4, 2) for D, n in ((16, 3), (7, 3))] \
    + [(2000, 4, D, n, 4096, k, k) for k in (2, 8, 64) for D, n in ((16, 3), (50, 1))]
# the second trip of the TransE emit kernels (16-lane teams: D <= 64), section C3
SECOND_TRIP_B = 65536 + 37
EXACT_SECOND_TRIP = [(500, 5, 16, 1, SECOND_TRIP_B, 4, 4), (500, 5, 64, 1, SECOND_TRIP_B, 4, 4)]


@functools.lru_cache(maxsize=2)
def exact_case(E, R, D, n, B):
    """-> dict(params, batch, want (the integer image), loss (oracle), share); margin 1, unscaled tables and distinct negatives
    as test_transe_sign_counts_are_the_exact_integer_sums has them."""
    rng = np.random.default_rng(seed_of("size-gate exact", E, R, D, n, B))
    params = oracle.init_params(oracle.TRANSE, E, R, D, D, seed=2)
    orc = oracle.Model("transe", E, R, D, D, margin=1.0, params=params)
    (bh, bt, br), share = batch_without_ties_by_group(orc, rng, E, R, B, n, 0, distinct=True, kinks=True)
    loss, _ = orc.grad(bh, bt, br, B, n)
    return dict(params=params, batch=(bh, bt, br), want=numpy_sign_counts(params, bh, bt, br, B, n, 1.0), loss=loss, share=share)


# (n, nr, foreign, D) at E = 97, R = 5, B = 4096: the form of test_transe_sign_count_gradient_matches_oracle
RELNEG_E, RELNEG_R, RELNEG_B, RELNEG_MARGIN = 97, 5, 4096, 0.8
RELNEG_CASES = [(n, nr, foreign, D) for n, nr, foreign in ((2, 2, 0.0), (3, 1, 0.3)) for D in (16, 50)]


@functools.lru_cache(maxsize=2)
def relneg_case(n, nr, foreign, D):
    E, R, B = RELNEG_E, RELNEG_R, RELNEG_B
    rng = np.random.default_rng(seed_of("size-gate relneg", D, n, nr))
    params = scaled_params("transe", E, R, D, seed=6)
    orc = oracle.Model("transe", E, R, D, D, margin=RELNEG_MARGIN, negative_rel=nr, params=params)
    (bh, bt, br), share = batch_without_ties_by_group(orc, rng, E, R, B, n, nr, foreign, kinks=True)
    loss, grads = oracle_grad(orc, bh, bt, br, B, n + nr)
    return dict(params=params, batch=(bh, bt, br), loss=loss, grads=grads, share=share)


def fused_graph():
    """(E, R, h, t, r): 9000 random triples over 500 entities and 6 relations; two batches per epoch give B >= 4096."""
    rng = np.random.default_rng(seed_of("size-gate fused graph"))
    E, R, T = 500, 6, 9000
    return E, R, rng.integers(0, E, T), rng.integers(0, E, T), rng.integers(0, R, T)


FUSED_NBATCHES, FUSED_NEG = 2, 5

# ---- C2: chunk lengths of the float-record segmented sum -----------------------------------------------------------------------
CHUNK_E, CHUNK_R, CHUNK_MARGIN = 3000, 5, 0.9
CHUNK_NEG = {"transe": 13, "transh": 12, "transd": 5}                     # 16 record slots per group for every model
CHUNK_SIZES = [(16383, 16), (16385, 32), (65537, 64)]                     # 2^18 - 16, 2^18 + 16, 2^20 + 16 records
CHUNK_CASES = [(model, D, B, chunk) for model in ("transe", "transh", "transd") for D in (8, 6) for B, chunk in CHUNK_SIZES]


def grad_case(tag, model, E, R, D, B, n, margin, foreign=0.0, plant=None):
    rng = np.random.default_rng(seed_of("size-gate", tag, model, D, B, n))
    params = scaled_params(model, E, R, D, seed=3)
    orc = oracle.Model(model, E, R, D, D, margin=margin, params=params)
    (bh, bt, br), share = batch_without_ties_by_group(orc, rng, E, R, B, n, 0, foreign)
    if plant is not None:
        plant(orc, rng, bh, bt, br)
    loss, grads = oracle_grad(orc, bh, bt, br, B, n)
    return dict(params=params, orc=orc, batch=(bh, bt, br), loss=loss, grads=grads, share=share)


@functools.lru_cache(maxsize=1)
def chunk_case(model, D, B):
    return grad_case("chunk", model, CHUNK_E, CHUNK_R, D, B, CHUNK_NEG[model], CHUNK_MARGIN)


# ---- C3: the second trip of the grid-capped kernels ------------------------------------------------------------------------------
TRIP_E, TRIP_R, TRIP_MARGIN = 500, 5, 0.9
MAX_LOSS_BLOCKS = 4096                                                    # csrc/engine.hpp kMaxLossBlocks
PAIR_TRIP_CASES = [(model, D) for model in ("transh", "transd") for D in (8, 68)]


def foreign_groups(bh, bt, br, B, N):
    """Groups with a negative that is not a single-entity corruption of its positive (what pair_emit_kernel defers)."""
    h, t, r = (x.reshape(1 + N, B) for x in (bh, bt, br))
    shaped = (r[1:] == r[:1]) & ((h[1:] == h[:1]) ^ (t[1:] == t[:1]))
    return np.nonzero(~shaped.all(0))[0]


def plant_second_trip_exits(orc, rng, bh, bt, br, B=SECOND_TRIP_B, first=MAX_LOSS_BLOCKS * 16):
    """n = 1.  Make sure that among the groups a 16-lane team takes on its second trip (b >= first) one has a foreign negative and
    another, sampler-shaped, has no active hinge: both `continue` exits of pair_emit_kernel.  Planted where the draw left none."""
    E, R = orc.params["ent_embeddings"].shape[0], orc.params["rel_embeddings"].shape[0]
    if not (foreign_groups(bh, bt, br, B, 1) >= first).any():
        b = first + 3
        bh[B + b], bt[B + b], br[B + b] = (bh[b] + 1) % E, (bt[b] + 1) % E, (br[b] + 1) % R
    for _ in range(200):
        hm = orc.hinge_margins(bh, bt, br, B, 1)[:, 0]
        assert np.abs(hm[first:]).min() > HINGE_TIE
        shaped = np.setdiff1d(np.arange(first, B), foreign_groups(bh, bt, br, B, 1))
        if (hm[shaped] < 0).any():
            return
        b = shaped[0]
        bh[B + b], bt[B + b], br[B + b] = rng.integers(0, E), bt[b], br[b]
        while bh[B + b] == bh[b] or abs(orc.hinge_margins(bh, bt, br, B, 1)[b, 0]) <= HINGE_TIE:
            bh[B + b] = rng.integers(0, E)
    raise AssertionError("no second-trip group without an active hinge")


@functools.lru_cache(maxsize=1)
def trip_case(model, D, foreign):
    return grad_case("trip", model, TRIP_E, TRIP_R, D, SECOND_TRIP_B, 1, TRIP_MARGIN, foreign,
                     plant=plant_second_trip_exits if foreign > 0 else None)
