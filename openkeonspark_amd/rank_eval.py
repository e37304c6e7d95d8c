"""Evaluation by ranking: top-k prediction, link and relation prediction, and ranking any triples against every entity or against
candidate lists -- all of it but the collectives over a sharded entity table, which are shard_eval's.  Functions take the Config
first; its public methods hold the documentation and dispatch here, and nothing here or in shard_eval calls back into them."""
import ctypes

import numpy as np

from . import _lib, parallel as par, shard_eval
from ._lib import KgeError
from .shard_eval import checked      # this rank's argument check, its exception kept for shard_eval.agree

# count columns 0..3 (raw, filtered, typed, filtered + typed) in the reference's accumulator names: (name, suffix)
COLUMNS = (("", ""), ("_filter", ""), ("", "_constrain"), ("_filter", "_constrain"))


def stem_sums(stem, columns):
    """The un-normalised accumulators of main_spark.py:430-448 (they add across slices of the triples) over count columns given
    in COLUMNS' order (the first two or all four), under the reference's names: `stem` r (tail side), l (head side) or rel."""
    d = {}
    for (name, suffix), cnt in zip(COLUMNS, columns):
        d[stem + name + "_tot" + suffix] = float((cnt < 10).sum())                    # Hits@10
        d[stem + "3" + name + "_tot" + suffix] = float((cnt < 3).sum())               # Hits@3
        d[stem + "1" + name + "_tot" + suffix] = float((cnt < 1).sum())               # Hits@1
        d[stem + name + "_rank" + suffix] = float((1 + cnt).sum())                    # MR
        d[stem + name + "_reci_rank" + suffix] = float((1.0 / (1 + cnt)).sum())       # MRR
    return d


def cand_sums(counts, sides=(0, 1)):
    """The accumulators of the ranked sides' counts [n, 2, 2] (candidate lists: raw, filtered; no _constrain names) or [n, 2, 4]."""
    d = {}
    for side, stem in ((0, "r"), (1, "l")):
        if side in sides:
            d.update(stem_sums(stem, counts[:, side].T))
    return d


def lp_sums(out, test_head=True):
    """The accumulators of link_prediction's rows [n, 2, 8] (columns 4.. are not counts) or rank_triples' [n, 2, 4]."""
    return cand_sums(out[:, :, :4], (0, 1) if test_head else (0,))


def rel_sums(out):
    """The accumulators of relation_prediction's rows [count, 4], under the stem "rel"."""
    return stem_sums("rel", out.T)


def normalise(sums, count):
    n = float(max(count, 1))
    return {k: v / n for k, v in sums.items()}


def all_reduce_sums(con, sums):
    """The accumulators of every rank added up (main_spark.py:430-448's reduction)."""
    import torch
    import torch.distributed as dist
    keys = sorted(sums)
    vec = torch.tensor([sums[k] for k in keys], dtype=torch.float64)
    if con.world_size > 1:
        if dist.get_backend(con._pg) == "nccl":
            vec = vec.to(con.device)
        shard_eval.all_reduce(con, vec, dist.ReduceOp.SUM)
    return dict(zip(keys, vec.cpu().tolist()))


def rank_slice(n, g, W):
    """The contiguous range (c0, c1) of n items that rank g of W takes (the static split of distribute_training.py:430-441)."""
    per = par.chunk_size(n, W)
    return min(g * per, n), min((g + 1) * per, n)


def replicated_counts(con, n, width, run):
    """The body of a collective on replicated tables, after agree: run(c0, c1, into) ranks this rank's slice of the n triples
    into its rows of a zeroed int64 device tensor [n, 2, width], and ONE SUM all-reduce merges the slices.  -> numpy [n, 2, width]."""
    import torch
    import torch.distributed as dist
    counts = torch.zeros((max(n, 1), 2, width), dtype=torch.int64, device=con.device)
    c0, c1 = rank_slice(n, con.rank, con.world_size)
    if c1 > c0:
        run(c0, c1, counts[c0:c1])
    shard_eval.all_reduce(con, counts, dist.ReduceOp.SUM)
    return counts[:n].cpu().numpy()


def sharded_in_group(con, what):
    """Is the entity table sharded?  Then the collective `what` needs the process group (no other rank can wait without one)."""
    import torch.distributed as dist
    sharded = con._sharded("ent_embeddings")
    if sharded and not dist.is_initialized():
        raise KgeError("%s over an entity table sharded across ranks needs the process group it was sharded over" % what)
    return sharded


def triple_ids(con, h, t, r):
    """h, t, r (1-D id arrays of one length) as a checked int32 device tensor [3, n]."""
    import torch
    host = np.stack([np.asarray(h).reshape(-1), np.asarray(t).reshape(-1), np.asarray(r).reshape(-1)]).astype(np.int32)
    con._check_ids(host)
    return torch.from_numpy(np.ascontiguousarray(host)).to(con.device)


def candidate_list(con, cand, n, name):
    """A candidate array ([n, C] or [C]; numpy / list / torch tensor on any device) -> (int32 device tensor, C, stride)."""
    import torch
    if torch.is_tensor(cand):
        if cand.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise KgeError("%s must hold integer ids, got %s" % (name, cand.dtype))
        dev = cand.to(device=con.device, dtype=torch.int32).contiguous()       # a device tensor stays on the device
    else:
        host = np.asarray(cand)
        if host.dtype.kind not in "iu" and host.size:
            raise KgeError("%s must hold integer ids, got %s" % (name, host.dtype))
        if host.size and (host.min() < -2 ** 31 or host.max() >= 2 ** 31):
            raise KgeError("%s: an id does not fit 32 bits" % name)
        dev = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(con.device)
    if dev.dim() == 1:
        return dev, int(dev.shape[0]), 0
    if dev.dim() == 2 and dev.shape[0] == n:
        return dev, int(dev.shape[1]), int(dev.shape[1])
    raise KgeError("%s must be [n, C] = [%d, C] or a shared list [C], got %s" % (name, n, list(dev.shape)))


def candidate_lists(con, what, n, tail_candidates, head_candidates):
    """The list arguments of rank_candidates (`what`: the caller's name, for the messages) -> (tail, head, n_cand, sides):
    tail / head = (int32 device tensor, stride) or None, sides the ranked ones of (0, 1)."""
    if tail_candidates is None and head_candidates is None:
        raise KgeError("%s: give tail_candidates, head_candidates or both" % what)
    tail = None if tail_candidates is None else candidate_list(con, tail_candidates, n, "tail_candidates")
    head = None if head_candidates is None else candidate_list(con, head_candidates, n, "head_candidates")
    if tail is not None and head is not None and tail[1] != head[1]:
        raise KgeError("%s: both lists must have the same number of candidates, got %d and %d" % (what, tail[1], head[1]))
    sides = [s for s, x in ((0, tail), (1, head)) if x is not None]
    return tail and (tail[0], tail[2]), head and (head[0], head[2]), (tail or head)[1], sides


def sampled_flags(test_head, type_constrained, filtered):
    return (_lib.RANKC_DRAWN | (0 if test_head else _lib.RANKC_NO_HEAD) | (_lib.RANKC_TYPED if type_constrained else 0) |
            (_lib.RANKC_FILTERED if filtered else 0))


def check_sampled(what, n_candidates):
    if int(n_candidates) < 0 or int(n_candidates) >= 2 ** 31:
        raise KgeError("%s: n_candidates must be in [0, 2^31), got %d" % (what, n_candidates))


def valid_rank_ids(con, sample, what):
    """The validation positives a check ranks, as an int32 device tensor [3, n] (h, t, r; ids checked): all V of valid2id.txt
    (read once, in file order), or with 0 < sample < V those at the indices floor(i V / sample).  Kept between calls."""
    import torch
    if getattr(con, "_valid_pos", None) is None:
        path = con.in_path if con.in_path.endswith("/") else con.in_path + "/"
        with open(path + "valid2id.txt") as f:
            tok = f.read().split()
        total = int(tok[0]) if tok else 0
        con._valid_pos = np.asarray(tok[1:1 + 3 * total], dtype=np.int64).reshape(total, 3).T.astype(np.int32)   # on disk: head, tail, relation
    valid = con._valid_pos
    total = valid.shape[1]
    sample = int(sample)
    if sample < 0:
        raise KgeError("%s: sample must be >= 0, got %d" % (what, sample))
    if 0 < sample < total:
        valid = valid[:, (np.arange(sample, dtype=np.int64) * total) // sample]
    else:
        sample = 0
    cached = getattr(con, "_valid_rank_dev", None)
    if cached is None or cached[0] != sample:
        host = np.ascontiguousarray(valid)
        con._check_ids(host)
        cached = con._valid_rank_dev = (sample, torch.from_numpy(host).to(con.device))
    return cached[1]


def rank_device(con, dev, test_head, into=None):
    """kge_rank_triples on an int32 device tensor [3, n] (h, t, r; ids already checked) -> int64 numpy [n, 2, 4]; with
    `into` (a contiguous int64 device tensor [n, 2, 4]) the counts are left there and nothing is copied back.  bf16 tables under
    set_bf16_evaluation("stored"), or whose float32 view cannot be made: kge_rank_triples_bf16 on the stored rows, the same counts."""
    import torch
    n = dev.shape[1]
    counts = into if into is not None else torch.empty((n, 2, 4), dtype=torch.int64, device=con.device)
    # (an empty tensor has no address and the entry point refuses null pointers: n == 0 still checks the files, on a spare row)
    ids, out = (dev, counts) if n else (torch.zeros((3, 1), dtype=torch.int32, device=con.device),
                                        torch.zeros((1, 2, 4), dtype=torch.int64, device=con.device))
    raw = con._bf16_full_eval_tables("rank_triples")
    fn, tabs = (con.lib.kge_rank_triples, (con._tab_ptrs,)) if raw is None else (con.lib.kge_rank_triples_bf16, raw)
    _lib.check(fn(ctypes.byref(con._desc), *tabs, ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n, 1 if test_head else 0,
                  out.data_ptr(), con._stream()), con.lib)
    return counts.cpu().numpy() if into is None else None


def rank_candidates_device(con, dev, tail, head, n_cand, flags, seed, first=0, into=None):
    """kge_rank_candidates on an int32 device tensor [3, n] (ids already checked); tail / head = (tensor, stride) or None.
    `first` is the global index of the first triple, for drawn lists (the hash is indexed by it: _lib.drawn_seed_at moves the
    seed there).  -> int64 numpy [n, 2, 2], or None with `into` (a device tensor).  Every caller uses this module-level name."""
    import torch
    n = dev.shape[1]
    counts = into if into is not None else torch.empty((n, 2, 2), dtype=torch.int64, device=con.device)
    spare = torch.zeros((3, 4), dtype=torch.int32, device=con.device)        # an empty tensor has no address
    ptr = lambda x: x.data_ptr() if x.numel() else spare.data_ptr()
    ids = dev if n else spare
    lists = [(None, 0) if side is None else (ptr(side[0]), side[1]) for side in (tail, head)]
    raw = con._bf16_eval_tables()      # stored bf16 tables are ranked from their own rows: no float32 view, the same counts
    fn, tabs = (con.lib.kge_rank_candidates, (con._tab_ptrs,)) if raw is None else (con.lib.kge_rank_candidates_bf16, raw)
    _lib.check(fn(ctypes.byref(con._desc), *tabs, ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(),
                  n, lists[0][0], lists[0][1], lists[1][0], lists[1][1], n_cand, flags, _lib.drawn_seed_at(seed, first),
                  counts.data_ptr() if n else spare.data_ptr(), con._stream()), con.lib)
    return counts.cpu().numpy() if into is None else None


def topk_queries(con, a, b, k, a_total, b_total):
    """Argument handling of the top-k methods: the k check, the two id arrays broadcast against each other and checked
    against [0, a_total) / [0, b_total) before any launch.  -> (a, b as int32 device tensors, n, on_device)."""
    import torch
    k = int(k)
    if not 1 <= k <= _lib.TOPK_MAX_K:
        raise KgeError("top-k prediction: k must be in [1, %d], got %d" % (_lib.TOPK_MAX_K, k))
    on_device = any(isinstance(x, torch.Tensor) and x.device.type != "cpu" for x in (a, b))
    if on_device:
        a, b = (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)) for x in (a, b))
        a, b = torch.broadcast_tensors(a.to(con.device).reshape(-1), b.to(con.device).reshape(-1))
        a = a.to(torch.int32).contiguous()
        b = b.to(torch.int32).contiguous()
        n = a.shape[0]
        if n:   # the ids index device tables directly: checked before any launch (four numbers come back)
            lim = torch.stack([a.min(), a.max(), b.min(), b.max()]).cpu().tolist()
            if lim[0] < 0 or lim[1] >= a_total or lim[2] < 0 or lim[3] >= b_total:
                raise KgeError("entity / relation id out of range in the top-k queries")
    else:
        ah, bh = np.broadcast_arrays(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1))
        n = ah.shape[0]
        if n and (ah.min() < 0 or ah.max() >= a_total or bh.min() < 0 or bh.max() >= b_total):
            raise KgeError("entity / relation id out of range in the top-k queries")
        a = torch.from_numpy(np.ascontiguousarray(ah, dtype=np.int32)).to(con.device)
        b = torch.from_numpy(np.ascontiguousarray(bh, dtype=np.int32)).to(con.device)
    return a, b, n, on_device


def topk_flags(filtered, type_constrained):
    return (_lib.TOPK_FILTERED if filtered else 0) | (_lib.TOPK_TYPED if type_constrained else 0)


def topk_call(con, fn, query_ptrs, n, k, flags, on_device, tabs=None):
    """`tabs`: the table arguments, where they are not the float32 tables (stored bf16 tables: the two addresses)."""
    import torch
    k = int(k)
    ids = torch.empty((n, k), dtype=torch.int32, device=con.device)
    scores = torch.empty((n, k), dtype=torch.float32, device=con.device)
    tabs = (con._tab_ptrs,) if tabs is None else tabs
    _lib.check(fn(ctypes.byref(con._desc), *tabs, *query_ptrs, n, k, flags, ids.data_ptr(), scores.data_ptr(), con._stream()), con.lib)
    return topk_result(ids, scores, on_device)


def topk_result(ids, scores, on_device):
    return (ids.long(), scores) if on_device else (ids.cpu().numpy().astype(np.int64), scores.cpu().numpy())


def top_k_entities(con, fixed, rel, k, head, filtered, type_constrained):
    import torch
    flags = topk_flags(filtered, type_constrained)
    if con._sharded("ent_embeddings"):
        queries, err = checked(lambda: topk_queries(con, fixed, rel, k, con.entTotal, con.relTotal))
        f, r, n, on_device = queries if err is None else (None, None, 0, False)
        return topk_result(*shard_eval.top_k_entities(con, f, r, n, k, err, head, flags), on_device)
    f, r, n, on_device = topk_queries(con, fixed, rel, k, con.entTotal, con.relTotal)
    side = torch.full((n,), 1 if head else 0, dtype=torch.int32, device=con.device)
    raw = con._bf16_full_eval_tables("top_k_heads" if head else "top_k_tails")      # stored bf16 rows: the same ids and score bits
    fn = con.lib.kge_topk_entities if raw is None else con.lib.kge_topk_entities_bf16
    return topk_call(con, fn, (f.data_ptr(), r.data_ptr(), side.data_ptr()), n, k, flags, on_device, tabs=raw)


def top_k_relations(con, h, t, k, filtered, type_constrained):
    if con._sharded("ent_embeddings"):
        raise KgeError("top-k relation prediction over an entity table sharded across ranks is not supported")
    h, t, n, on_device = topk_queries(con, h, t, k, con.entTotal, con.entTotal)
    return topk_call(con, con.lib.kge_topk_relations, (h.data_ptr(), t.data_ptr()), n, k, topk_flags(filtered, type_constrained), on_device)


def link_prediction(con, first, count, test_head):
    if count is None:
        count = con.lib.getTestTotal() - first
    if con._sharded("ent_embeddings"):
        out = shard_eval.link_prediction(con, first, count, test_head)
    else:
        out = np.zeros((count, 2, 8), dtype=np.int64)
        _lib.check(con.lib.kge_link_prediction(ctypes.byref(con._desc), con._tab_ptrs, first, count, 1 if test_head else 0,
                                               out.ctypes.data, con._stream()), con.lib)
    return out, normalise(lp_sums(out, test_head), count)


def link_prediction_distributed(con, test_head):
    total = con.lib.getTestTotal()
    if con._sharded("ent_embeddings"):
        return link_prediction(con, 0, total, test_head)[1]
    lo, hi = rank_slice(total, con.rank, con.world_size)
    out = link_prediction(con, lo, hi - lo, test_head)[0] if hi > lo else np.zeros((0, 2, 8), dtype=np.int64)
    return normalise(all_reduce_sums(con, lp_sums(out, test_head)), total)


def relation_prediction(con, first, count):
    if count is None:
        count = con.lib.getTestTotal() - first
    if con._sharded("ent_embeddings"):
        out = shard_eval.relation_prediction(con, first, count)
    else:
        out = np.zeros((count, 4), dtype=np.int64)
        _lib.check(con.lib.kge_relation_prediction(ctypes.byref(con._desc), con._tab_ptrs, first, count, out.ctypes.data,
                                                   con._stream()), con.lib)
    return out, normalise(rel_sums(out), count)


def relation_prediction_distributed(con):
    total = con.lib.getTestTotal()
    if con._sharded("ent_embeddings"):
        return relation_prediction(con, 0, total)[1]
    lo, hi = rank_slice(total, con.rank, con.world_size)
    out = relation_prediction(con, lo, hi - lo)[0] if hi > lo else np.zeros((0, 4), dtype=np.int64)
    return normalise(all_reduce_sums(con, rel_sums(out)), total)


def rank_triples(con, h, t, r, test_head):
    con._refuse_sharded_rank("rank_triples")
    counts = rank_device(con, triple_ids(con, h, t, r), test_head)
    return counts, normalise(lp_sums(counts, test_head), counts.shape[0])


def rank_ids_distributed(con, triples, test_head):
    """rank_triples_distributed / validation_link_prediction_distributed on a sharded table or with several ranks: `triples`
    returns the checked int32 device tensor [3, n]; whatever it raises on this rank is raised on every rank.  Replicated tables:
    the files checked without a launch (no triples), agree, this rank's slice by kge_rank_triples, one SUM all-reduce."""
    ids, err = checked(triples)
    if con._sharded("ent_embeddings"):
        counts = shard_eval.rank_triples(con, ids, err, test_head)
    else:
        if err is None:
            err = checked(lambda: rank_device(con, ids[:, :0], test_head))[1]
        n = int(ids.shape[1]) if err is None else -1
        per = max(1, int(con.lp_shard_query_bytes) // (2 * con.hidden_size * 4))
        shard_eval.agree(con, "rank_triples_distributed", err, (n, 1 if test_head else 0), [1, 2], "numbers of triples or test_head", per, where="")
        counts = replicated_counts(con, n, 4, lambda c0, c1, into: rank_device(con, ids[:, c0:c1].contiguous(), test_head, into=into))
    return counts, normalise(lp_sums(counts, test_head), counts.shape[0])


def rank_candidates(con, h, t, r, tail_candidates, head_candidates, filtered):
    con._refuse_sharded_candidates("rank_candidates")
    dev = triple_ids(con, h, t, r)
    tail, head, n_cand, sides = candidate_lists(con, "rank_candidates", dev.shape[1], tail_candidates, head_candidates)
    counts = rank_candidates_device(con, dev, tail, head, n_cand, _lib.RANKC_FILTERED if filtered else 0, 0)
    return counts, normalise(cand_sums(counts, sides), counts.shape[0])


def rank_candidates_distributed(con, h, t, r, tail_candidates, head_candidates, filtered):
    what = "rank_candidates_distributed"
    sharded, flags = sharded_in_group(con, what), _lib.RANKC_FILTERED if filtered else 0

    def check():
        dev = triple_ids(con, h, t, r)
        tail, head, n_cand, sides = candidate_lists(con, what, dev.shape[1], tail_candidates, head_candidates)
        if not sharded:
            rank_candidates_device(con, dev[:, :0], tail, head, n_cand, flags, 0)       # the arguments and the files, no launch
        return dev, tail, head, n_cand, sides
    args, err = checked(check)
    dev, tail, head, n_cand, sides = args if err is None else (None, None, None, 0, [])
    if sharded:
        counts = shard_eval.rank_candidates(con, dev, err, tail, head, n_cand, flags, 0, what)
    else:
        strides = [x[1] if x is not None else -1 for x in (tail, head)]
        n = int(dev.shape[1]) if err is None else -1
        shard_eval.agree(con, what, err, (n, flags, n_cand, *strides), [1, 2, 3, 4, 5], "triples, candidate counts, lists or flags", 0, where="")

        def run(c0, c1, into):      # a per-triple list starts at this slice's first triple; a shared list (stride 0) is whole
            part = [x and ((x[0][c0:c1] if x[1] else x[0]), x[1]) for x in (tail, head)]
            rank_candidates_device(con, dev[:, c0:c1].contiguous(), part[0], part[1], n_cand, flags, 0, into=into)
        counts = replicated_counts(con, n, 2, run)
    return counts, normalise(cand_sums(counts, sides), counts.shape[0])


def rank_triples_sampled(con, h, t, r, n_candidates, seed, test_head, type_constrained, filtered):
    con._refuse_sharded_candidates("rank_triples_sampled")
    check_sampled("rank_triples_sampled", n_candidates)
    flags = sampled_flags(test_head, type_constrained, filtered)
    counts = rank_candidates_device(con, triple_ids(con, h, t, r), None, None, int(n_candidates), flags, seed)
    return counts, normalise(cand_sums(counts, (0, 1) if test_head else (0,)), counts.shape[0])


def rank_sampled_distributed(con, what, triples, n_candidates, seed, test_head, type_constrained, filtered):
    """Drawn candidate lists on a sharded table (shard_eval.rank_candidates) or with several ranks: `triples` returns the checked
    int32 device tensor [3, n]; whatever it or the argument check raises on this rank is raised on every rank.  Replicated tables:
    the files checked without a launch, agree, this rank's slice (the seed moved to its first triple), one SUM all-reduce."""
    sharded = sharded_in_group(con, what)

    def check():
        check_sampled(what, n_candidates)
        dev, flags, s = triples(), sampled_flags(test_head, type_constrained, filtered), int(seed)
        if not sharded:
            rank_candidates_device(con, dev[:, :0], None, None, int(n_candidates), flags, s)       # the arguments and the files, no launch
        return dev, flags, s
    args, err = checked(check)
    dev, flags, seed = args if err is None else (None, 0, 0)
    if sharded:
        counts = shard_eval.rank_candidates(con, dev, err, None, None, n_candidates, flags, seed, what)
    else:
        n, n_cand = (int(dev.shape[1]), int(n_candidates)) if err is None else (-1, 0)
        shard_eval.agree(con, what, err, (n, flags, n_cand, seed & (2 ** 62 - 1)), [1, 2, 3, 4], "triples, candidate counts, seeds or flags", 0, where="")
        counts = replicated_counts(con, n, 2, lambda c0, c1, into: rank_candidates_device(
            con, dev[:, c0:c1].contiguous(), None, None, n_cand, flags, seed, first=c0, into=into))
    return counts, normalise(cand_sums(counts, (0, 1) if test_head else (0,)), counts.shape[0])


def validation_link_prediction(con, test_head, sample, candidates, seed, type_constrained):
    what = "validation_link_prediction"
    if int(candidates) < 0:
        raise KgeError("validation_link_prediction: candidates must be >= 0, got %d" % candidates)
    if int(candidates) > 0:
        con._refuse_sharded_candidates("validation_link_prediction(candidates=%d)" % candidates)
        check_sampled(what, candidates)
        flags = sampled_flags(test_head, type_constrained, True)
        counts = rank_candidates_device(con, valid_rank_ids(con, sample, what), None, None, int(candidates), flags, seed)
        return counts, normalise(cand_sums(counts, (0, 1) if test_head else (0,)), counts.shape[0])
    con._refuse_sharded_rank(what)
    counts = rank_device(con, valid_rank_ids(con, sample, what), test_head)
    return counts, normalise(lp_sums(counts, test_head), counts.shape[0])


def validation_link_prediction_distributed(con, test_head, sample, candidates, seed, type_constrained):
    what = "validation_link_prediction_distributed"
    cand = checked(lambda: int(candidates))[0]      # None: not a number, which `triples` reports on every rank
    if cand == 0:
        return rank_ids_distributed(con, lambda: valid_rank_ids(con, sample, what), test_head)

    def triples():
        if cand is None or cand < 0:
            raise KgeError("%s: candidates must be an integer >= 0, got %r" % (what, candidates))
        return valid_rank_ids(con, sample, what)
    return rank_sampled_distributed(con, what, triples, max(cand or 0, 0), seed, test_head, type_constrained, True)
