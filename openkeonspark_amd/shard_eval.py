"""Evaluation over an entity table sharded across ranks (`con._shard`).  Every function here is a collective: each rank calls it
the same number of times, and the order in which it enters torch.distributed collectives (fetch_rows, all_reduce, agree and the
`parallel` calls written out in it) is its contract with the other ranks.  top_k_entities, relation_prediction, rank_triples and
rank_candidates open with agree; test_step and link_prediction have no header step.  Functions take the Config first; its
public methods dispatch here, for ranking by way of rank_eval, which prepares the arguments; nothing here calls back into either."""
import ctypes

import numpy as np

from . import _lib, parallel as par
from ._lib import KgeError


def fetch_rows(con, ids, n):
    """Collective on a sharded entity table: the rows of the n global entity ids in `ids` (int32 device tensor), fetched from
    their owners by the sharded step's exchange (ids out, rows back).  -> (rows float32 [max(n, 1), D], slot_of int32 [n]:
    the row holding entity ids[i])."""
    import torch
    L, st, W, D, pg = con.lib, con._stream(), con.world_size, con.hidden_size, con._pg
    sh, dev, i32 = con._shard, con.device, torch.int32
    con.comm_fence("pg")
    counts = torch.zeros(W, dtype=i32, device=dev)
    cursor = torch.zeros(W, dtype=i32, device=dev)
    send_ids = torch.empty(max(n, 1), dtype=i32, device=dev)
    slot_of = torch.empty(max(n, 1), dtype=i32, device=dev)
    _lib.check(L.kge_shard_count(ids.data_ptr(), n, sh["chunk"], W, counts.data_ptr(), st), L)
    send, recv, gmax = par.exchange_counts_max(counts, pg)
    _lib.check(L.kge_shard_scatter(ids.data_ptr(), n, sh["chunk"], W, (ctypes.c_int64 * W)(*send), cursor.data_ptr(),
                                   send_ids.data_ptr(), slot_of.data_ptr(), st), L)
    n_recv = sum(recv)
    recv_ids = torch.empty(max(n_recv, 1), dtype=i32, device=dev)
    rows_out = torch.empty((max(n_recv, 1), D), dtype=torch.float32, device=dev)
    rows = torch.zeros((max(n, 1), D), dtype=torch.float32, device=dev)
    par.all_to_all_rows(recv_ids, send_ids, recv, send, pg, max_rows=gmax)
    _lib.check(L.kge_shard_gather_rows(con._tables[0].data_ptr(), recv_ids.data_ptr(), n_recv, sh["lo"], sh["chunk"], D,
                                       rows_out.data_ptr(), st), L)
    par.all_to_all_rows(rows, rows_out, send, recv, pg, max_rows=gmax)
    return rows, slot_of[:n]


def query_rows(con, ids, n):
    """fetch_rows, in query order: -> float32 [n, D], row i that of entity ids[i] (repeated ids repeat their row)."""
    rows, slot_of = fetch_rows(con, ids, n)
    return rows.index_select(0, slot_of.long())


def all_reduce(con, t, op):
    """In-place all-reduce of a device tensor on the process group (staged through the host for gloo)."""
    import torch.distributed as dist
    con.comm_fence("pg")
    if dist.get_backend(con._pg) == "nccl":
        dist.all_reduce(t, op=op, group=con._pg)
    else:
        h = t.cpu()
        dist.all_reduce(h, op=op, group=con._pg)
        t.copy_(h)


def checked(check):
    """This rank's own argument check, run before agree: -> (check(), None), or (None, what a bad argument or a missing file
    raised) for agree to raise as KgeError on every rank.  An exception that escaped here would leave the other ranks waiting."""
    try:
        return check(), None
    except (KgeError, ValueError, TypeError, OverflowError, OSError, RuntimeError, AttributeError) as e:
        return None, e


def agree(con, what, err, fields, same, differ, per, where=" on a sharded entity table"):
    """The first collective of a call whose arguments can be wrong: one all-gather of the int64 header [ok, *fields, per], so
    that a bad call raises KgeError on every rank and leaves none waiting in a later collective.  `err` is what this
    rank's own argument check raised (or None), `same` the header columns that must be equal on all ranks, `differ` their
    names in the message.  -> (the headers int64 [W, 2 + len(fields)], the smallest `per` of any rank)."""
    import torch
    hdr = torch.tensor([0 if err else 1, *fields, per], dtype=torch.int64, device=con.device)
    con.comm_fence("pg")
    allh = torch.empty((con.world_size, hdr.numel()), dtype=torch.int64, device=con.device)
    par.all_gather_chunks(allh.view(-1), hdr, con._pg)
    allh = allh.cpu().numpy()
    on = "%s%s: " % (what, where)
    if err is not None:
        raise KgeError(on + "%s" % err) from err
    if not allh[:, 0].all():
        raise KgeError(on + "rank(s) %s passed invalid arguments" % np.nonzero(allh[:, 0] == 0)[0].tolist())
    if (allh[:, same] != allh[0, same]).any():
        raise KgeError(on + "the ranks passed different " + differ)
    return allh, int(allh[:, -1].min())


def test_step(con, host):
    import torch
    n = host.shape[1]
    ids = torch.from_numpy(np.ascontiguousarray(host[:2].reshape(-1))).to(con.device)    # the n heads, then the n tails
    rows, slot_of = fetch_rows(con, ids, 2 * n)
    out = torch.empty(n, dtype=torch.float32, device=con.device)
    if n:
        slots = slot_of.view(2, n)
        rel = torch.from_numpy(np.ascontiguousarray(host[2])).to(con.device)
        desc = con._desc_with(ent_total=rows.shape[0])       # entity ids are slots of the fetched rows
        ptrs = _lib.table_ptrs([rows.data_ptr()] + [t.data_ptr() for t in con._tables[1:]])
        _lib.check(con.lib.kge_predict(ctypes.byref(desc), ptrs, slots[0].data_ptr(), slots[1].data_ptr(), rel.data_ptr(), n,
                                       out.data_ptr(), con._stream()), con.lib)
    con.trainModel.predict = out
    return out.cpu().numpy()


def link_prediction(con, first, count, test_head):
    """Config.link_prediction on a sharded entity table: every rank ranks the test triples against its own rows [lo, hi), the
    counts are summed and the arg-min keys minimised across ranks, then resolved as kge_link_prediction does."""
    import torch
    import torch.distributed as dist
    L, st, D = con.lib, con._stream(), con.hidden_size
    lo, hi = con._shard["lo"], con._shard["hi"]
    th = 1 if test_head else 0
    out = np.zeros((count, 2, 8), dtype=np.int64)
    per = max(1, int(con.lp_shard_query_bytes) // (2 * D * 4))
    for c0 in range(first, first + count, per):
        n = min(per, first + count - c0)
        ids = torch.empty(2 * n, dtype=torch.int32, device=con.device)
        _lib.check(L.kge_test_entity_ids(c0, n, ids.data_ptr(), st), L)
        query = query_rows(con, ids, 2 * n)       # [2n, D]: the h and t rows of each triple
        counts = torch.empty((n, 2, 4), dtype=torch.int64, device=con.device)
        keys = torch.empty_like(counts)
        _lib.check(L.kge_link_prediction_range(ctypes.byref(con._desc), con._tab_ptrs, lo, hi - lo, query.data_ptr(), c0, n, th,
                                               counts.data_ptr(), keys.data_ptr(), st), L)
        all_reduce(con, counts, dist.ReduceOp.SUM)
        all_reduce(con, keys, dist.ReduceOp.MIN)
        _lib.check(L.kge_link_prediction_finish(c0, n, th, counts.data_ptr(), keys.data_ptr(), out[c0 - first:].ctypes.data, st), L)
    return out


def top_k_entities(con, f, r, n, k, err, head, flags):
    """Config.top_k_tails / top_k_heads on a sharded entity table.  f / r are this rank's n queries (fixed entity, relation) as
    checked int32 device tensors, `err` what their check raised (or None; k is then in range).  -> device (ids int32 [n, k],
    scores float32 [n, k]).  The ranks first agree on a header (query count, k, side, flags, validity).  Then all ranks' queries
    are taken in chunks: their fixed rows are fetched from the owners, each query's k best among this rank's rows [lo, hi) are
    selected as packed keys (kge_topk_entities_range), each requester is sent the key lists of its own queries only, and the W
    lists received for each of this rank's queries are merged (kge_topk_merge_keys)."""
    import torch
    L, st, W, D, dev, pg = con.lib, con._stream(), con.world_size, con.hidden_size, con.device, con._pg
    lo, hi = con._shard["lo"], con._shard["hi"]
    if err is None:      # the arguments, and the evaluation files the flags need, checked without a launch (no queries)
        k = int(k)
        err = checked(lambda: _lib.check(L.kge_topk_entities_range(ctypes.byref(con._desc), con._tab_ptrs, lo, hi - lo, None, None,
                                                                   None, None, 0, k, flags, None, st), L))[1]
    n, kk = (n, k) if err is None else (0, -1)
    per = max(1, int(con.topk_shard_query_bytes) // (4 * D + 8 * max(kk, 1)))
    allh, per = agree(con, "top-k prediction", err, (n, kk, 1 if head else 0, flags), [2, 3, 4], "k, side or flags", per)
    ns = allh[:, 1]
    off = np.concatenate([[0], np.cumsum(ns)]).tolist()
    N, me = off[-1], con.rank
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    if N:
        # every rank's queries (fixed, relation), rank-major: padded to the largest count for one all-gather
        nmax = int(ns.max())
        q = torch.zeros((nmax, 2), dtype=torch.int32, device=dev)
        if n:
            q[:n, 0] = f
            q[:n, 1] = r
        allq = torch.empty((W, nmax, 2), dtype=torch.int32, device=dev)
        par.all_gather_chunks(allq.view(-1), q.view(-1), pg)
        allq = torch.cat([allq[g, :int(ns[g])] for g in range(W)])
        gf, gr = allq[:, 0].contiguous(), allq[:, 1].contiguous()
        side = torch.full((N,), 1 if head else 0, dtype=torch.int32, device=dev)
        for c0 in range(0, N, per):
            c1 = min(N, c0 + per)
            m = c1 - c0
            query = query_rows(con, gf[c0:c1], m)         # [m, D]: the fixed rows of the chunk's queries
            keys = torch.empty((m, k), dtype=torch.int64, device=dev)
            _lib.check(L.kge_topk_entities_range(ctypes.byref(con._desc), con._tab_ptrs, lo, hi - lo, query.data_ptr(),
                                                 gf[c0:].data_ptr(), gr[c0:].data_ptr(), side[c0:].data_ptr(), m, k, flags,
                                                 keys.data_ptr(), st), L)
            del query
            # rank g's queries are [off[g], off[g+1]): their key lists in this chunk go back to g alone
            send = [max(0, min(c1, off[g + 1]) - max(c0, off[g])) for g in range(W)]
            mine = send[me]
            got = torch.empty((max(W * mine, 1), k), dtype=torch.int64, device=dev)
            con.comm_fence("pg")
            par.all_to_all_rows(got, keys, [mine] * W, send, pg, max_rows=max(send))
            if mine:      # [W][mine][k]: one key list per source rank
                o0 = max(c0, off[me]) - off[me]
                _lib.check(L.kge_topk_merge_keys(got.data_ptr(), mine, W, k, ids[o0].data_ptr(), scores[o0].data_ptr(), st), L)
    return ids, scores


def relation_prediction(con, first, count):
    """Config.relation_prediction on a sharded entity table.  The ranks first agree on a header (validity, first, count,
    triples per round).  Then rank g takes the g-th contiguous slice of [first, first+count) in rounds of at most `per`
    triples: the h / t rows come from their owners (query_rows, which every rank joins in every round, with no ids once its
    slice is done) and kge_relation_prediction_rows writes the slice's rows of a zeroed [count, 4]; one SUM all-reduce merges
    them.  -> raw int64 [count, 4]."""
    import torch
    import torch.distributed as dist
    L, st, W, D, dev = con.lib, con._stream(), con.world_size, con.hidden_size, con.device
    if not dist.is_initialized():      # no process group, so no other rank can be waiting for this one
        raise KgeError("relation prediction on a sharded entity table needs the process group it was sharded over")

    def check():
        f, c = int(first), int(count)
        if f < 0 or c < 0:
            raise KgeError("relation prediction: bad range (first %d, count %d)" % (f, c))
        # the arguments and the evaluation files, checked without a launch: the range's end, then no triples
        _lib.check(L.kge_relation_prediction_rows(ctypes.byref(con._desc), con._tab_ptrs, None, f + c, 0, None, st), L)
        return f, c
    span, err = checked(check)
    first, count = span if err is None else (-1, -1)
    per = max(1, int(con.lp_shard_query_bytes) // (2 * D * 4))
    _, per = agree(con, "relation prediction", err, (first, count), [1, 2], "first or count", per)
    cs = par.chunk_size(count, W)
    lo = first + min(con.rank * cs, count)
    hi = first + min((con.rank + 1) * cs, count)
    counts = torch.zeros((max(count, 1), 4), dtype=torch.int64, device=dev)
    for r0 in range(0, cs, per):
        c0 = min(lo + r0, hi)
        n = min(per, hi - c0)
        ids = torch.empty(max(2 * n, 1), dtype=torch.int32, device=dev)
        _lib.check(L.kge_test_entity_ids(c0, n, ids.data_ptr(), st), L)
        query = query_rows(con, ids, 2 * n)       # [2n, D]: the h and t rows of each triple
        if n:
            _lib.check(L.kge_relation_prediction_rows(ctypes.byref(con._desc), con._tab_ptrs, query.data_ptr(), c0, n,
                                                      counts[c0 - first].data_ptr(), st), L)
        del query
    all_reduce(con, counts, dist.ReduceOp.SUM)
    return counts[:count].cpu().numpy()


def rank_triples(con, ids, err, test_head):
    """Config.rank_triples_distributed / validation_link_prediction_distributed on a sharded entity table.  `ids` is the int32
    device tensor [3, n] (h, t, r; ids already checked) or None, `err` what this rank's own argument check raised (or None).
    The ranks first agree on a header (validity, n, test_head, triples per round); the evaluation files are checked before it,
    without a launch.  In rounds of `per` triples the 2 per h and t rows come from their owners (query_rows, laid out
    [per][2][D]) and kge_rank_triples_range ranks the round against this rank's rows [lo, hi) into its slice of one
    [n, 2, 4] device tensor; ONE SUM all-reduce of that tensor follows the last round.  -> int64 numpy [n, 2, 4]."""
    import torch
    import torch.distributed as dist
    L, st, D, dev = con.lib, con._stream(), con.hidden_size, con.device
    if not dist.is_initialized():      # no process group, so no other rank can be waiting for this one
        raise KgeError("rank_triples_distributed on a sharded entity table needs the process group it was sharded over")
    lo, hi = con._shard["lo"], con._shard["hi"]
    th = 1 if test_head else 0
    if err is None:      # the arguments and the evaluation files, checked without a launch (no triples)
        err = checked(lambda: _lib.check(L.kge_rank_triples_range(ctypes.byref(con._desc), con._tab_ptrs, lo, hi - lo, None, None, None,
                                                                  None, 0, th, None, st), L))[1]
    n = int(ids.shape[1]) if err is None else -1
    per = max(1, int(con.lp_shard_query_bytes) // (2 * D * 4))
    _, per = agree(con, "rank_triples_distributed", err, (n, th), [1, 2], "numbers of triples or test_head", per)
    counts = torch.zeros((max(n, 1), 2, 4), dtype=torch.int64, device=dev)
    for c0 in range(0, n, per):
        m = min(per, n - c0)
        pairs = ids[:2, c0:c0 + m].t().contiguous().view(-1)      # h0, t0, h1, t1, ...
        query = query_rows(con, pairs, 2 * m)                      # [m][2][D]: the raw h and t row of each triple
        _lib.check(L.kge_rank_triples_range(ctypes.byref(con._desc), con._tab_ptrs, lo, hi - lo, query.data_ptr(),
                                            ids[0, c0:].data_ptr(), ids[1, c0:].data_ptr(), ids[2, c0:].data_ptr(), m, th,
                                            counts[c0].data_ptr(), st), L)
        del query
    all_reduce(con, counts, dist.ReduceOp.SUM)
    return counts[:n].cpu().numpy()


def rank_candidates(con, ids, err, tail, head, n_cand, flags, seed, what="rank_candidates_distributed"):
    """Config.rank_candidates_distributed / rank_triples_sampled_distributed on a sharded entity table, whose process group the
    caller has found.  `ids` is the int32 device tensor [3, n] (h, t, r; checked) or None, `err` what this rank's own argument
    check raised (or None); tail / head = (int32 device tensor, stride) or None; with KGE_RANKC_DRAWN in `flags` both are None
    and `seed` draws the lists.  The ranks first agree on a header (validity, n, C, flags, which sides have a list, their strides,
    the seed, triples per round); the arguments and the evaluation files are checked before it, without a launch.  Then, in
    rounds of `per` triples, the 2 per h and t rows come from their owners (query_rows, laid out [per][2][D]) and
    kge_rank_candidates_range ranks the round against this rank's rows [lo, hi) into its slice of one [n, 2, 2] device tensor: a
    round's per-triple lists start at c0 x stride, and its drawn lists are indexed by the global triple (_lib.drawn_seed_at moves
    the seed there).  ONE SUM all-reduce of that tensor closes the call: every rank compares against the same target score bits
    and counts the candidates it owns, so the sum is kge_rank_candidates over the whole table.  -> int64 numpy [n, 2, 2]."""
    import torch
    import torch.distributed as dist
    L, st, D, dev = con.lib, con._stream(), con.hidden_size, con.device
    lo, hi = con._shard["lo"], con._shard["hi"]
    spare = torch.zeros((3, 4), dtype=torch.int32, device=dev)        # an empty tensor has no address
    ptr = lambda x, off=0: (x.view(-1)[off:] if off else x).data_ptr() if x.numel() > off else spare.data_ptr()

    def check():      # -> the header
        C, fl = int(n_cand), int(flags)
        lists = [(None, 0) if side is None else (ptr(side[0]), int(side[1])) for side in (tail, head)]
        # the arguments and the evaluation files, checked without a launch (no triples)
        _lib.check(L.kge_rank_candidates_range(ctypes.byref(con._desc), con._tab_ptrs, lo, hi - lo, None, spare.data_ptr(),
                                               spare.data_ptr(), spare.data_ptr(), 0, lists[0][0], lists[0][1], lists[1][0],
                                               lists[1][1], C, fl, 0, spare.data_ptr(), st), L)
        sides = (1 if tail is not None else 0) | (2 if head is not None else 0)
        return int(ids.shape[1]), C, fl, sides, lists[0][1], lists[1][1], int(seed) & (2 ** 62 - 1)
    if err is None:
        header, err = checked(check)
    if err is not None:
        header = (-1, 0, 0, 0, 0, 0, 0)
    n, n_cand, flags = header[:3]
    per = max(1, int(con.lp_shard_query_bytes) // (2 * D * 4))
    _, per = agree(con, what, err, header, [1, 2, 3, 4, 5, 6, 7], "numbers of triples or candidates, flags, lists or seeds", per)
    counts = torch.zeros((max(n, 1), 2, 2), dtype=torch.int64, device=dev)
    for c0 in range(0, n, per):
        m = min(per, n - c0)
        pairs = ids[:2, c0:c0 + m].t().contiguous().view(-1)      # h0, t0, h1, t1, ...
        query = query_rows(con, pairs, 2 * m)                      # [m][2][D]: the raw h and t row of each triple
        round_lists = [(None, 0) if side is None else (ptr(side[0], c0 * int(side[1])), int(side[1])) for side in (tail, head)]
        _lib.check(L.kge_rank_candidates_range(ctypes.byref(con._desc), con._tab_ptrs, lo, hi - lo, query.data_ptr(),
                                               ids[0, c0:].data_ptr(), ids[1, c0:].data_ptr(), ids[2, c0:].data_ptr(), m,
                                               round_lists[0][0], round_lists[0][1], round_lists[1][0], round_lists[1][1],
                                               n_cand, flags, _lib.drawn_seed_at(seed, c0), counts[c0].data_ptr(), st), L)
        del query
    all_reduce(con, counts, dist.ReduceOp.SUM)
    return counts[:n].cpu().numpy()
