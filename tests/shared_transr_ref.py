"""fp64 reference of "TransR on relation-grouped chunks" (include/kge_mi355.h) for the TransR shared-negatives tests: the lists
are expanded into the ordinary batch they stand for (shared_transh_ref.expand: a masked pair is spelled as the positive itself,
whose hinge is the margin and whose gradient is exactly zero) and put through torch_ref.loss_and_grads("transr", ...) in fp64.
No device, no engine."""
import numpy as np

import shared_transh_ref as tref

TABLES = ("ent_embeddings", "rel_embeddings", "transfer_matrix")


def make_tables(E, R, De, Dr, seed):
    rng = np.random.default_rng(seed)
    return {"ent_embeddings": rng.normal(0, 0.1, (E, De)).astype(np.float32), "rel_embeddings": rng.normal(0, 0.1, (R, Dr)).astype(np.float32),
            "transfer_matrix": rng.normal(0, 0.1, (R, De * Dr)).astype(np.float32)}


def conditions(params, bh, bt, br, n_pos, N, masked, margin, De, Dr):
    """(min |v| over the unmasked pairs, min |e| over every element of every scored triple, active [n_pos, N]) in fp64: the
    positive's matrix for every negative (TransR.py:57-60)."""
    ent, rel = params["ent_embeddings"].astype(np.float64), params["rel_embeddings"].astype(np.float64)
    mat = params["transfer_matrix"].astype(np.float64).reshape(len(rel), De, Dr)
    l2n = lambda x: x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12))
    rp = br[:n_pos]
    M = mat[rp]                                                             # [n_pos, De, Dr]
    proj = lambda ids, m: l2n(np.einsum("bi,bij->bj", ent[ids], m))
    rn = l2n(rel[rp])
    ep = proj(bh[:n_pos], M) + rn - proj(bt[:n_pos], M)
    p = np.abs(ep).sum(-1)
    min_sign, min_kink = float(np.abs(ep).min()), np.inf
    active = np.zeros((n_pos, N), dtype=bool)
    for k in range(N):
        o = (k + 1) * n_pos
        e = proj(bh[o:o + n_pos], M) + rn - proj(bt[o:o + n_pos], M)
        v = p - np.abs(e).sum(-1) + margin
        live = ~masked[:, k]
        if live.any():
            min_kink = min(min_kink, float(np.abs(v[live]).min()))
            min_sign = min(min_sign, float(np.abs(e[live]).min()))
        active[:, k] = live & (v >= 0)
    return min_kink, min_sign, active


def listed_rows(h, t, r, cand, chunks, active, pair):
    """{table: sorted rows the definition gives a gradient}: h_b and t_b of a positive with an active pair, a candidate with an
    active pair, and the relation (rel_embeddings row and matrix) of a chunk with one."""
    ent, rel = set(), set()
    for j, (lo, n) in enumerate(np.asarray(chunks).tolist()):
        act = active[lo:lo + n]
        if n == 0 or not act.any():
            continue
        rel.add(int(r[lo]))
        for b in np.nonzero(act.any(1))[0]:
            ent.update((int(h[lo + b]), int(t[lo + b])))
        ent.update(int(c) for c in np.asarray(cand[j])[act.any(0)])
    rel = np.array(sorted(rel), dtype=np.int64)
    return {"ent_embeddings": np.array(sorted(ent), dtype=np.int64), "rel_embeddings": rel, "transfer_matrix": rel}


def reference(params, h, t, r, cand, pair, chunks, margin, denom, De, Dr):
    """The definition in fp64 -> dict(loss, grads {table: float64}, listed {table: rows with a gradient}, min_kink, min_sign,
    active, batch (bh, bt, br)).  Outside the listed rows autograd leaves at most the cancellation residue of the masked pairs
    (the positive scored twice, + g and - g summed in another order): asserted below 1e-12, and set to the exact zero it stands
    for."""
    from torch_ref import loss_and_grads
    n_pos, N = pair.shape
    bh, bt, br = tref.expand(h, t, r, cand, pair, chunks, n_pos)
    masked = (pair & 2) != 0
    loss, g = loss_and_grads("transr", params, bh, bt, br, n_pos, N, margin, De, Dr)
    s = n_pos * N / denom                                                   # the reference is a mean over n_pos N hinges
    loss = loss * s - masked.sum() * margin / denom                         # a masked pair adds nothing and stays in the denominator
    min_kink, min_sign, active = conditions(params, bh, bt, br, n_pos, N, masked, margin, De, Dr)
    listed = listed_rows(h, t, r, cand, chunks, active, pair)
    grads = {}
    for k in TABLES:
        gk = g[k] * s
        rest = np.setdiff1d(np.arange(len(gk)), listed[k])
        assert np.abs(gk[rest]).max(initial=0.0) <= 1e-12, (k, np.abs(gk[rest]).max())
        gk[rest] = 0.0
        grads[k] = gk
    return dict(loss=loss, grads=grads, listed=listed, min_kink=min_kink, min_sign=min_sign, active=active, batch=(bh, bt, br))


def row_report(got, want, rtol, listed):
    """Per table: (rows outside `listed` that are not exactly zero in `got`, the largest |difference| / (rtol * the row's fp64
    magnitude) over the listed rows, their number)."""
    out = {}
    for name in TABLES:
        ref = np.asarray(want[name], dtype=np.float64)
        g = np.asarray(got[name], dtype=np.float64).reshape(ref.shape)
        rows = listed[name]
        rest = np.setdiff1d(np.arange(len(ref)), rows)
        mag = np.abs(ref[rows]).max(1)
        off = np.abs(g[rows] - ref[rows]).max(1)
        assert (mag > 0).all(), name
        out[name] = (int((g[rest] != 0).any(1).sum()), float((off / (rtol * mag)).max()) if len(rows) else 0.0, len(rows))
    return out
