"""numpy fp64 restatement of "TransD on relation-grouped chunks" (include/kge_mi355.h): the forward, the integer count vectors
and the float gradient records of kge_transd_emit_records_shared_chunks, with their keys in the float-record row space.  Shared
by the TransD shared-negatives tests; no device, no engine."""
import numpy as np

from shared_transh_ref import chunk_of_positions, expand, l2n_parts, normalize_bwd      # noqa: F401  (the lists are TransH's)

TABLES = ("ent_embeddings", "rel_embeddings", "rel_transfer", "ent_transfer")      # the order of the kernel's `tables`


def hub_space(E, R, n_pos_total):
    """(hub_base, hub_k) of the row space a TransD step of n_pos_total positives keys its float records in (models.hip
    record_space): ent [0, E) | ent_transfer [E, 2 E) | hub_k copies of { rel_embeddings [R] | rel_transfer [R] }."""
    k = (2 * int(n_pos_total)) // (2 * R * 64) if R > 0 else 1
    return 2 * E, min(max(k, 1), 4096)


def project(x, xp, rp):
    """side_project<KGE_TRANSD>: a = x . x_p, x^ = l2n(x + a r_p)."""
    a = (x * xp).sum(-1)
    xn, inv, uc = l2n_parts(x + a[:, None] * rp[None, :])
    return xn, a, inv, uc


def side_backward(x, xp, xn, a, inv, uc, G, rp):
    """(gradients of the ent_embeddings rows, of the ent_transfer rows, the rows' shares of d/dr_p) of side_backward<KGE_TRANSD>."""
    gxp = normalize_bwd(xn, G, inv, uc)
    d = gxp @ rp
    return gxp + d[:, None] * xp, d[:, None] * x, a[:, None] * gxp


def forward(ent, rel, relp, entp, h, t, r, cand, pair, chunks, margin, denom, n_pos_total):
    """The definition in fp64.  ent / rel / relp / entp: fp32 tables (ent_embeddings, rel_embeddings, rel_transfer, ent_transfer);
    h, t, r: [n_pos] in sorted order; cand: [cap, N]; pair: uint8 [n_pos, N]; chunks: [cap, 2] (first sorted position, length).
    Returns a dict:
      keys     int64 [M], M = 4 n_pos + cap (2 N + 2): the key of every record (-1 = none), in the kernel's record order
      records  float64 [M, D]
      counts   int64 [M, D]: the count vectors, on the ent_embeddings and rel_embeddings records (the others have none: zeros)
      loss     float
      min_kink min |v| over the unmasked pairs, min_sign min |e| over every element of every scored triple
      active   bool [n_pos, N]"""
    ent, rel, relp, entp = (np.asarray(x, dtype=np.float64) for x in (ent, rel, relp, entp))
    E, D = ent.shape
    R = len(rel)
    h = np.asarray(h, dtype=np.int64); t = np.asarray(t, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    n_pos, N = pair.shape
    cap = len(chunks)
    M = 4 * n_pos + cap * (2 * N + 2)
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
        rn, inv_r, uc_r = l2n_parts(rel[rho][None, :])
        rn, rp = rn[0], relp[rho]
        hh, tt = h[lo:hi], t[lo:hi]
        ids_ok = (hh >= 0) & (hh < E) & (tt >= 0) & (tt < E)
        ih, it = np.where(ids_ok, hh, 0), np.where(ids_ok, tt, 0)
        Hn, a_h, inv_h, uc_h = project(ent[ih], entp[ih], rp)
        Tn, a_t, inv_t, uc_t = project(ent[it], entp[it], rp)
        c = cand[j].astype(np.int64)
        ok = (c >= 0) & (c < E)
        ic = np.where(ok, c, 0)
        Cn, a_c, inv_c, uc_c = project(ent[ic], entp[ic], rp)
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
        m_rel, m_relp, m_c0 = 4 * n_pos + j, 4 * n_pos + cap + j, 4 * n_pos + 2 * cap + j * N
        acw = np.zeros(D)
        any_ent = False
        for G, idx, xn, a, inv, uc, ids, m0, step in ((G_h, ih, Hn, a_h, inv_h, uc_h, hh, lo, n_pos), (G_t, it, Tn, a_t, inv_t, uc_t, tt, 2 * n_pos + lo, n_pos),
                                                      (G_c, ic, Cn, a_c, inv_c, uc_c, c, m_c0, cap * N)):
            nz = np.abs(G).sum(1) > 0
            g, gp, share = side_backward(ent[idx], entp[idx], xn, a, inv, uc, unit * G, rp)
            blk, blk_p = slice(m0, m0 + len(G)), slice(m0 + step, m0 + step + len(G))
            counts[blk] = G
            recs[blk] = g * nz[:, None]
            recs[blk_p] = gp * nz[:, None]
            keys[blk] = np.where(nz, ids, -1)
            keys[blk_p] = np.where(nz, E + ids, -1)      # with its row's key, even where d = 0
            acw += share[nz].sum(0)
            any_ent = any_ent or bool(nz.any())
        hub = hub_base + (j % hub_k) * 2 * R
        counts[m_rel] = G_r
        if np.abs(G_r).sum() > 0:
            keys[m_rel] = hub + rho
            recs[m_rel] = normalize_bwd(rn[None, :], unit * G_r[None, :], inv_r, uc_r)[0]
        if any_ent:
            keys[m_relp] = hub + R + rho
            recs[m_relp] = acw      # r_p is used raw: no normalise-backward
    return dict(keys=keys, records=recs, counts=counts, loss=loss * unit, min_kink=min_kink, min_sign=min_sign, active=active)


def table_gradients(keys, records, E, R, n_pos_total):
    """{table name: float64 [rows, D]} over the four tables: the records summed per key, the hub copies folded onto their rows."""
    hub_base, _ = hub_space(E, R, n_pos_total)
    keys = np.asarray(keys, dtype=np.int64)
    records = np.asarray(records, dtype=np.float64)
    D = records.shape[1]
    out = {"ent_embeddings": np.zeros((E, D)), "ent_transfer": np.zeros((E, D)), "rel_embeddings": np.zeros((R, D)), "rel_transfer": np.zeros((R, D))}
    live = keys >= 0
    ent = live & (keys < E)
    entp = live & (keys >= E) & (keys < hub_base)
    np.add.at(out["ent_embeddings"], keys[ent], records[ent])
    np.add.at(out["ent_transfer"], keys[entp] - E, records[entp])
    off = (keys - hub_base) % (2 * R)
    is_rel = live & (keys >= hub_base) & (off < R)
    is_relp = live & (keys >= hub_base) & (off >= R)
    np.add.at(out["rel_embeddings"], off[is_rel], records[is_rel])
    np.add.at(out["rel_transfer"], off[is_relp] - R, records[is_relp])
    return out


def touched_rows(keys, E, R, n_pos_total):
    """{table name: sorted rows that have a record}."""
    hub_base, _ = hub_space(E, R, n_pos_total)
    keys = np.asarray(keys, dtype=np.int64)
    live = keys[keys >= 0]
    off = (live[live >= hub_base] - hub_base) % (2 * R)
    return {"ent_embeddings": np.unique(live[live < E]), "ent_transfer": np.unique(live[(live >= E) & (live < hub_base)] - E),
            "rel_embeddings": np.unique(off[off < R]), "rel_transfer": np.unique(off[off >= R] - R)}
