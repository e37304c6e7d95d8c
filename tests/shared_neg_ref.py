"""numpy restatement of the shared-negatives definition (include/kge_mi355.h, "TransE on negatives SHARED by a chunk of
positives"): the counter hashes in uint64, and the forward / records of kge_transe_emit_records_shared in fp64.  Shared by the
shared-negatives tests; no device, no engine."""
import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def mix(z):
    u = np.uint64
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=u)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        return z ^ (z >> u(31))


def step_key(seed, step):
    return int(mix(np.uint64((int(seed) + (int(step) + 1) * GAMMA) & M64)))


def _draw(S, counter, n):
    u = np.uint64
    with np.errstate(over="ignore"):
        z = mix(u(S) + (np.asarray(counter, dtype=u) + u(1)) * u(GAMMA))
        return ((z >> u(32)) * u(n)) >> u(32)


def candidates(seed, step, n_chunks, N, ent_total, first_chunk=0):
    """int32 [n_chunks, N]: candidate k of chunk j."""
    S = step_key(seed, step)
    j = (np.arange(n_chunks, dtype=np.uint64) + np.uint64(first_chunk))[:, None]
    k = np.arange(N, dtype=np.uint64)[None, :]
    return _draw(S, (j << np.uint64(8)) | k, ent_total).astype(np.int32)


def side_draws(seed, step, n_pos, N, first_position=0):
    """int64 [n_pos, N]: v in [0, 1000) of the pair (position p, candidate k)."""
    S = step_key(seed, step)
    p = (np.arange(n_pos, dtype=np.uint64) + np.uint64(first_position))[:, None]
    k = np.arange(N, dtype=np.uint64)[None, :]
    return _draw(S, (p << np.uint64(8)) | np.uint64(128) | k, 1000).astype(np.int64)


def sides(v, r, bern_prob=None):
    """uint8 [n_pos, N]: 0 = new tail, 1 = new head -- (float)v < 500.0f, or < the relation's Bernoulli value, means a new tail."""
    prob = np.float32(500.0) if bern_prob is None else np.asarray(bern_prob, dtype=np.float32)[np.asarray(r)][:, None]
    return np.where(v.astype(np.float32) < prob, 0, 1).astype(np.uint8)


def l2n(x):
    return x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12))


def forward(ent, rel, h, t, r, cand, pair, P, margin, denom):
    """The definition in fp64.  ent / rel: fp32 tables; h, t, r: [n_pos]; cand: [n_chunks, N]; pair: uint8 [n_pos, N].
    Returns a dict:
      keys     int64 [3 n_pos + n_chunks N]  the destination key of every record (-1 = none), in the kernel's record order
      records  int64 [3 n_pos + n_chunks N, D]  the count vectors
      loss     float
      min_kink min |p - n + margin| over the unmasked pairs, min_sign min |e| over every element of every scored triple
      active   bool [n_pos, N]"""
    ent = np.asarray(ent, dtype=np.float64); rel = np.asarray(rel, dtype=np.float64)
    E, D = ent.shape
    n_pos, N = pair.shape
    n_chunks = -(-n_pos // P)
    H, T, Rn = l2n(ent[h]), l2n(ent[t]), l2n(rel[r])
    ep = H + Rn - T
    p_score = np.abs(ep).sum(-1)
    sp = np.sign(ep).astype(np.int64)
    keys = np.full(3 * n_pos + n_chunks * N, -1, dtype=np.int64)
    recs = np.zeros((3 * n_pos + n_chunks * N, D), dtype=np.int64)
    active = np.zeros((n_pos, N), dtype=bool)
    loss, min_kink, min_sign = 0.0, np.inf, np.inf
    scored_pos = np.zeros(n_pos, dtype=bool)
    for j in range(n_chunks):
        lo, hi = j * P, min((j + 1) * P, n_pos)
        c = cand[j].astype(np.int64)
        ok = (c >= 0) & (c < E)
        C = l2n(ent[np.where(ok, c, 0)])                                    # [N, D]
        pb = pair[lo:hi]                                                    # [Pc, N]
        live = ((pb & 2) == 0) & ok[None, :]
        head = (pb & 1) == 1
        e_tail = (H[lo:hi] + Rn[lo:hi])[:, None, :] - C[None, :, :]         # new tail: h^ + r^ - c^
        e_head = C[None, :, :] + (Rn[lo:hi] - T[lo:hi])[:, None, :]         # new head: c^ + r^ - t^
        e = np.where(head[:, :, None], e_head, e_tail)                      # [Pc, N, D]
        v = p_score[lo:hi, None] - np.abs(e).sum(-1) + margin
        act = live & (v >= 0)
        active[lo:hi] = act
        loss += float(v[act].sum())
        if live.any():
            min_kink = min(min_kink, float(np.abs(v[live]).min()))
            min_sign = min(min_sign, float(np.abs(e[live]).min()))
        scored_pos[lo:hi] = live.any(1)
        s = np.sign(e).astype(np.int64) * act[:, :, None]
        g = np.where(head[:, :, None], -s, s)                               # the candidate's share
        base = 3 * n_pos + j * N
        recs[base:base + N] = g.sum(0)
        keys[base:base + N] = np.where(act.any(0), c, -1)
        cnt = act.sum(1)[:, None]
        recs[lo:hi] = -(s * ~head[:, :, None]).sum(1) + cnt * sp[lo:hi]                          # h: -s of every new tail
        recs[n_pos + lo:n_pos + hi] = (s * head[:, :, None]).sum(1) - cnt * sp[lo:hi]            # t: +s of every new head
        recs[2 * n_pos + lo:2 * n_pos + hi] = -s.sum(1) + cnt * sp[lo:hi]                        # r: -s of every active pair
    for slot, ids in enumerate((np.asarray(h, dtype=np.int64), np.asarray(t, dtype=np.int64), np.asarray(r, dtype=np.int64) + E)):
        blk = slice(slot * n_pos, (slot + 1) * n_pos)
        keys[blk] = np.where(np.abs(recs[blk]).sum(1) > 0, ids, -1)
    if scored_pos.any():
        min_sign = min(min_sign, float(np.abs(ep[scored_pos]).min()))
    return dict(keys=keys, records=recs, loss=loss / denom, min_kink=min_kink, min_sign=min_sign, active=active)


def reduce(keys, records):
    """(touched rows increasing, their summed count vectors) -- what kge_transe_reduce_records leaves."""
    live = keys >= 0
    rows, inv = np.unique(keys[live], return_inverse=True)
    counts = np.zeros((len(rows), records.shape[1]), dtype=np.int64)
    np.add.at(counts, inv, records[live])
    return rows, counts


def expand(h, t, r, cand, pair, P, stride):
    """The ordinary batch the lists stand for (Base.cpp:109-139 layout, `stride` slots per round): negative k of positive b is
    (h_b, c_k, r_b) for a new tail, (c_k, t_b, r_b) for a new head, at b + (k + 1) * stride."""
    n_pos, N = pair.shape
    bh = np.zeros(stride * (1 + N), dtype=np.int32); bt = np.zeros_like(bh); br = np.zeros_like(bh)
    bh[:n_pos], bt[:n_pos], br[:n_pos] = h, t, r
    c = cand[np.arange(n_pos) // P]                      # [n_pos, N]
    head = (pair & 1) == 1
    for k in range(N):
        o = (k + 1) * stride
        bh[o:o + n_pos] = np.where(head[:, k], c[:, k], h)
        bt[o:o + n_pos] = np.where(head[:, k], t, c[:, k])
        br[o:o + n_pos] = r
    return bh, bt, br
