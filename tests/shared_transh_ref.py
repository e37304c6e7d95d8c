"""numpy fp64 restatement of "TransH on relation-grouped chunks" (include/kge_mi355.h): the forward, the integer count vectors
and the float gradient records of kge_transh_emit_records_shared_chunks, with their keys in the float-record row space.  Shared
by the TransH shared-negatives tests; no device, no engine."""
import numpy as np


def hub_space(E, R, n_pos_total):
    """(hub_base, hub_k) of the row space a TransH step of n_pos_total positives keys its float records in (models.hip
    record_space): entity rows, then hub_k copies of { rel_embeddings [R] | normal_vectors [R] }."""
    k = (2 * int(n_pos_total)) // (2 * R * 64) if R > 0 else 1
    return E, min(max(k, 1), 4096)


def l2n_parts(x):
    """(x^, 1 / norm, unclipped) of l2n(x) = x / sqrt(max(sum x^2, 1e-12)), rows of a 2-d array."""
    ss = (x * x).sum(-1)
    uc = ss >= 1e-12
    inv = 1.0 / np.sqrt(np.where(uc, ss, 1e-12))
    return x * inv[..., None], inv, uc


def normalize_bwd(y, gy, inv, uc):
    d = np.where(uc, (y * gy).sum(-1), 0.0)
    return inv[..., None] * (gy - d[..., None] * y)


def project(x, wn):
    a = x @ wn
    xn, inv, uc = l2n_parts(x - a[:, None] * wn[None, :])
    return xn, a, inv, uc


def side_backward(x, xn, a, inv, uc, G, wn):
    """(row gradients, the rows' shares of d/dw^) of side_backward<KGE_TRANSH> (models_dev.hpp)."""
    gxp = normalize_bwd(xn, G, inv, uc)
    d = gxp @ wn
    return gxp - d[:, None] * wn[None, :], -(d[:, None] * x + a[:, None] * gxp)


def forward(ent, rel, nrm, h, t, r, cand, pair, chunks, margin, denom, n_pos_total):
    """The definition in fp64.  ent / rel / nrm: fp32 tables; h, t, r: [n_pos] in sorted order; cand: [cap, N]; pair: uint8
    [n_pos, N]; chunks: [cap, 2] (first sorted position, length).  Returns a dict:
      keys     int64 [M], M = 2 n_pos + cap (N + 2): the key of every record (-1 = none), in the kernel's record order
      records  float64 [M, D]
      counts   int64 [M, D]: the count vectors (the normal-vector record has none: zeros)
      loss     float
      min_kink min |v| over the unmasked pairs, min_sign min |e| over every element of every scored triple
      active   bool [n_pos, N]"""
    ent = np.asarray(ent, dtype=np.float64); rel = np.asarray(rel, dtype=np.float64); nrm = np.asarray(nrm, dtype=np.float64)
    E, D = ent.shape
    R = len(rel)
    h = np.asarray(h, dtype=np.int64); t = np.asarray(t, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    n_pos, N = pair.shape
    cap = len(chunks)
    M = 2 * n_pos + cap * (N + 2)
    hub_base, hub_k = hub_space(E, R, n_pos_total)
    unit = 1.0 / denom
    keys = np.full(M, -1, dtype=np.int64)
    recs = np.zeros((M, D))
    counts = np.zeros((M, D), dtype=np.int64)
    active = np.zeros((n_pos, N), dtype=bool)
    loss, min_kink, min_sign = 0.0, np.inf, np.inf
    for j, (lo, n) in enumerate(np.asarray(chunks).tolist()):
        if n == 0:
            continue
        hi = lo + n
        rho = int(r[lo])
        if not 0 <= rho < R:
            continue
        wn, inv_w, uc_w = l2n_parts(nrm[rho][None, :])
        rn, inv_r, uc_r = l2n_parts(rel[rho][None, :])
        wn, rn = wn[0], rn[0]
        hh, tt = h[lo:hi], t[lo:hi]
        ids_ok = (hh >= 0) & (hh < E) & (tt >= 0) & (tt < E)
        xh, xt = ent[np.where(ids_ok, hh, 0)], ent[np.where(ids_ok, tt, 0)]
        Hn, a_h, inv_h, uc_h = project(xh, wn)
        Tn, a_t, inv_t, uc_t = project(xt, wn)
        c = cand[j].astype(np.int64)
        ok = (c >= 0) & (c < E)
        xc = ent[np.where(ok, c, 0)]
        Cn, a_c, inv_c, uc_c = project(xc, wn)
        ep = Hn + rn[None, :] - Tn
        p_score = np.abs(ep).sum(-1)
        sp = np.sign(ep).astype(np.int64)
        pb = pair[lo:hi]
        live = ((pb & 2) == 0) & ok[None, :] & ids_ok[:, None]
        head = (pb & 1) == 1
        e = np.where(head[:, :, None], Cn[None, :, :] + (rn[None, :] - Tn)[:, None, :], (Hn + rn[None, :])[:, None, :] - Cn[None, :, :])
        v = p_score[:, None] - np.abs(e).sum(-1) + margin
        act = live & (v >= 0)
        active[lo:hi] = act
        loss += float(v[act].sum())
        if live.any():
            min_kink = min(min_kink, float(np.abs(v[live]).min()))
            min_sign = min(min_sign, float(np.abs(e[live]).min()), float(np.abs(ep[live.any(1)]).min()))
        s = np.sign(e).astype(np.int64) * act[:, :, None]
        cnt = act.sum(1)[:, None]
        G_h = -(s * ~head[:, :, None]).sum(1) + cnt * sp
        G_t = (s * head[:, :, None]).sum(1) - cnt * sp
        G_r = (-s.sum(1) + cnt * sp).sum(0)
        G_c = np.where(head[:, :, None], -s, s).sum(0)
        m_rel, m_nrm, m_c0 = 2 * n_pos + j, 2 * n_pos + cap + j, 2 * n_pos + 2 * cap + j * N
        acw = np.zeros(D)
        for G, x, xn, a, inv, uc, ids, m0 in ((G_h, xh, Hn, a_h, inv_h, uc_h, hh, lo), (G_t, xt, Tn, a_t, inv_t, uc_t, tt, n_pos + lo),
                                              (G_c, xc, Cn, a_c, inv_c, uc_c, c, m_c0)):
            nz = np.abs(G).sum(1) > 0
            g, w_share = side_backward(x, xn, a, inv, uc, unit * G, wn)
            blk = slice(m0, m0 + len(G))
            counts[blk] = G
            recs[blk] = g * nz[:, None]
            keys[blk] = np.where(nz, ids, -1)
            acw += w_share[nz].sum(0)
        any_ent = bool((keys[lo:hi] >= 0).any() or (keys[n_pos + lo:n_pos + hi] >= 0).any() or (keys[m_c0:m_c0 + N] >= 0).any())
        hub = hub_base + (j % hub_k) * 2 * R
        counts[m_rel] = G_r
        if np.abs(G_r).sum() > 0:
            keys[m_rel] = hub + rho
            recs[m_rel] = normalize_bwd(rn[None, :], unit * G_r[None, :], inv_r, uc_r)[0]
        if any_ent:
            keys[m_nrm] = hub + R + rho
            recs[m_nrm] = normalize_bwd(wn[None, :], acw[None, :], inv_w, uc_w)[0]
    return dict(keys=keys, records=recs, counts=counts, loss=loss * unit, min_kink=min_kink, min_sign=min_sign, active=active)


def table_gradients(keys, records, E, R, n_pos_total):
    """{table name: float64 [rows, D]}: the records summed per key, the hub copies folded onto their rows."""
    hub_base, _ = hub_space(E, R, n_pos_total)
    keys = np.asarray(keys, dtype=np.int64)
    records = np.asarray(records, dtype=np.float64)
    D = records.shape[1]
    out = {"ent_embeddings": np.zeros((E, D)), "rel_embeddings": np.zeros((R, D)), "normal_vectors": np.zeros((R, D))}
    live = keys >= 0
    ent = live & (keys < hub_base)
    np.add.at(out["ent_embeddings"], keys[ent], records[ent])
    off = (keys - hub_base) % (2 * R)
    is_rel = live & ~ent & (off < R)
    is_nrm = live & ~ent & (off >= R)
    np.add.at(out["rel_embeddings"], off[is_rel], records[is_rel])
    np.add.at(out["normal_vectors"], off[is_nrm] - R, records[is_nrm])
    return out


def touched_rows(keys, E, R, n_pos_total):
    """{table name: sorted rows that have a record}."""
    hub_base, _ = hub_space(E, R, n_pos_total)
    keys = np.asarray(keys, dtype=np.int64)
    live = keys[keys >= 0]
    off = (live[live >= hub_base] - hub_base) % (2 * R)
    return {"ent_embeddings": np.unique(live[live < hub_base]), "rel_embeddings": np.unique(off[off < R]),
            "normal_vectors": np.unique(off[off >= R] - R)}


def chunk_of_positions(chunks, n_pos):
    """int64 [n_pos]: the chunk of every sorted position (a table that covers every position once)."""
    out = np.full(n_pos, -1, dtype=np.int64)
    for j, (lo, n) in enumerate(np.asarray(chunks).tolist()):
        out[lo:lo + n] = j
    assert (out >= 0).all()
    return out


def expand(h, t, r, cand, pair, chunks, stride):
    """The ordinary batch the lists stand for (`stride` slots per round): negative k of sorted position b is (h_b, c_k, r_b) for a
    new tail, (c_k, t_b, r_b) for a new head, at b + (k + 1) * stride; a MASKED pair is spelled as the positive itself."""
    n_pos, N = pair.shape
    c = np.asarray(cand)[chunk_of_positions(chunks, n_pos)]
    head, masked = (pair & 1) == 1, (pair & 2) != 0
    bh = np.zeros(stride * (1 + N), dtype=np.int32); bt = np.zeros_like(bh); br = np.zeros_like(bh)
    bh[:n_pos], bt[:n_pos], br[:n_pos] = h, t, r
    for k in range(N):
        o = (k + 1) * stride
        bh[o:o + n_pos] = np.where(masked[:, k] | ~head[:, k], h, c[:, k])
        bt[o:o + n_pos] = np.where(masked[:, k] | head[:, k], t, c[:, k])
        br[o:o + n_pos] = r
    return bh, bt, br
