"""Host restatements for the in-chunk candidates of relation-grouped shared negatives (include/kge_mi355.h, "In-chunk
candidates"), shared by tests/test_gpu_shared_in_chunk_step.py and tools/shared_in_chunk_seeds.py; no device, no engine.

host_lists      the whole draw of one step in numpy -- order, chunk table, drawn candidates (typed or not), in-chunk candidates,
                sides and masks -- from the step's positives and the training set.
reference_step  one training step of any of the four models in fp64 from lists N + K wide: the existing restatements
                (test_gpu_shared_emit_chunks.forward_chunks, shared_transh_ref, shared_transd_ref, shared_transr_ref,
                torch_ref.loss_and_grads) take their widths from the lists, so they are called as they stand."""
import numpy as np

import shared_neg_ref as ref
import shared_transd_ref as dref
import shared_transh_ref as tref
import shared_transr_ref as rref

TABLES = {"transe": ("ent_embeddings", "rel_embeddings"), "transh": ("ent_embeddings", "rel_embeddings", "normal_vectors"),
          "transd": dref.TABLES, "transr": rref.TABLES}


def derived_type_lists(h, t, r, R):
    """(head_off, head_ids, tail_off, tail_ids): every relation's distinct heads and tails of the given triples, increasing -- the
    lists Config.init_evaluation_from_arrays(..., derive_types=True) derives when these are all the triples there are."""
    h, t, r = (np.asarray(x, dtype=np.int64) for x in (h, t, r))
    out = ()
    for ids in (h, t):
        lists = [np.unique(ids[r == k]) for k in range(R)]
        out += (np.cumsum([0] + [len(x) for x in lists]).astype(np.int64), np.concatenate(lists).astype(np.int64))
    return out


def host_lists(h, t, r, P, E, R, N, K, seed, step, train, bern_prob=None, type_lists=None):
    """(h2, t2, r2, cand int32 [n_chunks, N + K], pair uint8 [n_pos, N + K], perm, chunks [n_chunks, 2]) of one step.  train: the set
    of training triples (h, t, r); bern_prob: float32 [R] with setBern(1), else None; type_lists: (head_off, head_ids, tail_off,
    tail_ids) with typed candidates, else None."""
    from openkeonspark_amd.train_paths import shared_in_chunk_candidates, shared_relation_chunks
    u = np.uint64
    h, t, r = (np.asarray(x, dtype=np.int64) for x in (h, t, r))
    perm, chunks, n_chunks = shared_relation_chunks(r, P, R)
    chunks = chunks[:n_chunks]
    h2, t2, r2 = h[perm], t[perm], r[perm]
    Nt = N + K
    S, G = u(ref.step_key(seed, step)), u(ref.GAMMA)
    rho = r2[chunks[:, 0]]
    valid = (rho >= 0) & (rho < R)
    with np.errstate(over="ignore"):
        key = (np.arange(n_chunks, dtype=u)[:, None] << u(8)) | np.arange(Nt, dtype=u)[None, :]
        v = ((ref.mix(S + ((key | u(128)) + u(1)) * G) >> u(32)) * u(1000)) >> u(32)
        draw = ref.mix(S + (key + u(1)) * G) >> u(32)
        prob = np.full(n_chunks, 500.0, dtype=np.float32)
        if bern_prob is not None:
            prob[valid] = np.asarray(bern_prob, dtype=np.float32)[rho[valid]]
        new_tail = v.astype(np.float32) < prob[:, None]
        cand = ((draw * u(E)) >> u(32)).astype(np.int32)
        if type_lists is not None:
            head_off, head_ids, tail_off, tail_ids = type_lists
            for j in np.flatnonzero(valid):
                for k in range(N):
                    off, ids = (tail_off, tail_ids) if new_tail[j, k] else (head_off, head_ids)
                    lst = ids[off[rho[j]]:off[rho[j] + 1]]
                    if len(lst):
                        cand[j, k] = lst[int((draw[j, k] * u(len(lst))) >> u(32))]
    sides = np.where(new_tail, 0, 1).astype(np.uint8)
    cand[:, N:] = shared_in_chunk_candidates(h2, t2, chunks, n_chunks, sides, N, K, seed, step, valid=valid)
    pair = np.zeros((len(h), Nt), dtype=np.uint8)
    for j, (b0, n) in enumerate(chunks.tolist()):
        for k in range(Nt):
            c = int(cand[j, k])
            for b in range(b0, b0 + n):
                tri = (int(h2[b]), c, int(rho[j])) if new_tail[j, k] else (c, int(t2[b]), int(rho[j]))
                masked = bool(valid[j]) and tri in train
                if k >= N:
                    masked = masked or c < 0 or c == (int(t2[b]) if new_tail[j, k] else int(h2[b]))
                pair[b, k] = sides[j, k] | (2 if masked else 0)
    return h2, t2, r2, cand, pair, perm, chunks


def reference_step(model, opt, s0, lists, lr_t, alpha, E, R, margin, adam_eps):
    """The state the definition gives from s0 (tables, and m<i> / v<i> or a<i> slots) for a step on `lists` = (h2, t2, r2, cand, pair,
    chunks): dict(loss, state, listed {table: rows}, excused {table: rows near a kink}, near, min_kink).  opt: "SGD", "LazyAdam" or
    "Adagrad" on the listed rows; TransR: SGD on the whole tables."""
    from torch_ref import loss_and_grads, near_kink_rows
    from test_gpu_adagrad import adagrad_rule_fp32
    import test_gpu_lazy_rows
    from test_gpu_lazy_rows import adam_rule_fp32
    from test_gpu_shared_emit_chunks import forward_chunks
    h, t, r, cand, pair, chunks = lists
    B, Nt = pair.shape
    denom = B * Nt
    tables = TABLES[model]
    params = {name: s0[name] for name in tables}
    De, Dr = params["ent_embeddings"].shape[1], params["rel_embeddings"].shape[1]
    masked = (pair & 2) != 0
    if model == "transr":
        want = rref.reference(params, h, t, r, cand, pair, chunks, margin, denom, De, Dr)
        loss, listed, (bh, bt, br) = want["loss"], want["listed"], want["batch"]
        g = {name: want["grads"][name].reshape(s0[name].shape) for name in tables}
    else:
        bh, bt, br = tref.expand(h, t, r, cand, pair, chunks, B)
        loss, g = loss_and_grads(model, params, bh, bt, br, B, Nt, margin, De, Dr)
        loss -= masked.sum() * margin / denom
        if model == "transe":
            want = forward_chunks(params["ent_embeddings"], params["rel_embeddings"], h, t, r, cand, pair, chunks, margin, denom)
            keys = want["keys"]
            listed = {"ent_embeddings": np.unique(keys[(keys >= 0) & (keys < E)]), "rel_embeddings": np.unique(keys[keys >= E]) - E}
        elif model == "transh":
            want = tref.forward(params["ent_embeddings"], params["rel_embeddings"], params["normal_vectors"], h, t, r, cand, pair, chunks,
                                margin, denom, B)
            listed = tref.touched_rows(want["keys"], E, R, B)
        else:
            want = dref.forward(params["ent_embeddings"], params["rel_embeddings"], params["rel_transfer"], params["ent_transfer"], h, t, r,
                                cand, pair, chunks, margin, denom, B)
            listed = dref.touched_rows(want["keys"], E, R, B)
        assert abs(loss - want["loss"]) <= 1e-9 * max(abs(loss), 1e-9)      # (the two restatements of the definition agree)
    out = {}
    for i, name in enumerate(tables):
        p0, gi, rows = s0[name], g[name].astype(np.float32), listed[name]
        rest = np.setdiff1d(np.arange(len(p0)), rows)
        assert np.abs(g[name][rest]).max(initial=0.0) <= 1e-12               # no gradient outside the listed rows
        p1 = p0.copy()
        if model == "transr":
            p1 = (p0 - np.float32(alpha) * gi).astype(np.float32)
        elif opt == "LazyAdam":
            m1, v1 = s0["m%d" % i].copy(), s0["v%d" % i].copy()
            eps0, test_gpu_lazy_rows.EPS = test_gpu_lazy_rows.EPS, adam_eps      # (the restatement reads its module's constant)
            try:
                p1[rows], m1[rows], v1[rows], _ = adam_rule_fp32(p0[rows], m1[rows], v1[rows], gi[rows], lr_t)
            finally:
                test_gpu_lazy_rows.EPS = eps0
            out["m%d" % i], out["v%d" % i] = m1, v1
        elif opt == "Adagrad":
            a1 = s0["a%d" % i].copy()
            p1[rows], a1[rows], _ = adagrad_rule_fp32(p0[rows], a1[rows], gi[rows], alpha)
            out["a%d" % i] = a1
        else:
            p1[rows] = (p0[rows] - np.float32(alpha) * gi[rows]).astype(np.float32)
        out[name] = p1
    excused, near = near_kink_rows(model, params, bh, bt, br, B, Nt, De, Dr, tol=1e-6)
    return dict(loss=loss, state=out, listed=listed, excused=excused, near=near, min_kink=want["min_kink"])
