"""The paths of a training step and the two data-parallel layouts.  Functions take the Config first; `Config.train_step` picks
the path from its step plan (step_plan.py) and dispatches here.  Which optimizer a touched-rows path ends in is decided in one
place, `RowsRule`; the dense paths (count image, fp32 gradient tables) end in Config.apply_counts / apply_gradients.
"""
import ctypes
import os

import numpy as np

from . import _lib, parallel as par
from ._lib import KgeError


class RowsRule(object):
    """The optimizer of the touched-rows paths -- SGD, lazy Adam, Adagrad or row-wise Adagrad -- as a host-side dispatch: which C entry point each
    of the three row-wise applications goes to, with which slot tables and which rate arguments.  Made by
    Config._refresh_pointers (it holds table and slot pointers) ; alpha and lazy Adam's lr_t are read from the Config at call
    time.  The SGD entry points are kernels of their own (atomic adds, a fused reduce-apply), not a third case of the device's
    row rule, so the split stays on the host."""

    def __init__(self, con):
        L = con.lib
        self.con = con
        self.kind = kind = con._plan.optimizer
        self.bf16 = bool(con._bf16)      # bf16 table storage: the listed-rows application alone, through its own entry points
        self.tabs = None if self.bf16 else con._tab_ptrs
        self.ent, self.rel = [t.data_ptr() for t in con._tables[:2]] if len(con._tables) >= 2 else (0, 0)
        if kind == "lazy_adam":
            self._fb_rows, self._float_records, self._listed_rows = \
                L.kge_forward_backward_adam_rows, L.kge_float_records_apply_adam, L.kge_transe_apply_rows_adam_lazy
            self.slot_ptrs = (con._adam_m_ptrs, con._adam_v_ptrs)
            self.row_slots = (con._adam_m[0].data_ptr(), con._adam_m[1].data_ptr(), con._adam_v[0].data_ptr(), con._adam_v[1].data_ptr())
        elif kind == "adagrad":
            self._fb_rows, self._float_records, self._listed_rows = \
                L.kge_forward_backward_adagrad_rows, L.kge_float_records_apply_adagrad, L.kge_transe_apply_rows_adagrad
            self.slot_ptrs = (con._adagrad_ptrs,)
            self.row_slots = (con._adagrad_acc[0].data_ptr(), con._adagrad_acc[1].data_ptr())
        elif kind == "row_adagrad":     # one accumulator per table row: [rows] floats where Adagrad has a table
            self._fb_rows, self._float_records, self._listed_rows = \
                L.kge_forward_backward_rowadagrad_rows, L.kge_float_records_apply_rowadagrad, L.kge_transe_apply_rows_rowadagrad
            self.slot_ptrs = (con._rowadagrad_ptrs,)
            self.row_slots = (con._rowadagrad_acc[0].data_ptr(), con._rowadagrad_acc[1].data_ptr())
        else:
            self._fb_rows, self._float_records, self._listed_rows = \
                L.kge_forward_backward_sgd_rows, L.kge_float_records_apply, L.kge_transe_apply_rows_sgd
            self.slot_ptrs = self.row_slots = ()
        if self.bf16:
            self._fb_rows = self._float_records = None      # (the float-record paths read fp32 tables)
            self._listed_rows = L.kge_transe_apply_rows_rowadagrad_bf16 if kind == "row_adagrad" else L.kge_transe_apply_rows_sgd_bf16

    def _rate(self):
        """The rate arguments every entry point of this rule takes after its data: lr_t and Adam's constants, or alpha."""
        con = self.con
        if self.kind == "lazy_adam":
            return float(con._adam_lr_t()), con.adam_beta1, con.adam_beta2, con.adam_epsilon
        return (float(con.alpha),)

    def forward_backward_rows(self, dev, n_pos, n_neg, stride, denom):
        """Forward / backward of a batch and the rule on the rows it touches, in place from float records, in one call."""
        con = self.con
        _lib.check(self._fb_rows(ctypes.byref(con._desc), self.tabs, *self.slot_ptrs, dev[0].data_ptr(), dev[1].data_ptr(),
                                 dev[2].data_ptr(), n_pos, n_neg, stride, denom, *self._rate(), con._loss.data_ptr(),
                                 con._stream()), con.lib)

    def apply_float_records(self, rec, dst, n_records, n_pos_total, n_neg):
        """The rule on the rows that `n_records` gathered float gradient records (rows `rec`, destination keys `dst`) name."""
        con = self.con
        _lib.check(self._float_records(ctypes.byref(con._desc), self.tabs, *self.slot_ptrs, rec.data_ptr(), dst.data_ptr(),
                                       n_records, n_pos_total, n_neg, *self._rate(), con._stream()), con.lib)

    def apply_listed_rows(self, desc, rows, counts, n_rows, max_rows, denom, live=None):
        """The rule on the rows listed in `rows` (device pointers: the list, its int32 sign counts, its length) of the row space
        `desc` describes, over this Config's TransE tables and slot tables.  live (lazy Adam only): an int32 tensor, listed row
        i is processed only where live[i] != 0; None = every listed row."""
        con = self.con
        mask = (live.data_ptr() if live is not None else None,) if self.kind == "lazy_adam" else ()
        if self.bf16:       # stochastic rounding: the hash takes the seed and the global step of this update
            mask = (ctypes.c_uint64(con._table_seed), ctypes.c_uint64(con.global_step))
        _lib.check(self._listed_rows(ctypes.byref(desc), self.ent, self.rel, *self.row_slots, rows, counts, n_rows, max_rows,
                                     denom, *self._rate(), *mask, con._stream()), con.lib)

    def reduce_apply(self, desc, rec, dst, n, buf, denom, fused_ok):
        """`n` int8 records (`rec`, destination rows `dst`) -> per-row sign counts in buf's rows / row_counts / n_rows -> the rule
        on those rows.  SGD with fused_ok: reduce + apply in one pass, only chunk-boundary rows go through the compact count
        image.  (Lazy Adam and both Adagrads are not linear in the gradient: they need a row's complete sum.)"""
        con = self.con
        rows, counts, n_rows = buf["rows"].data_ptr(), buf["row_counts"].data_ptr(), buf["n_rows"].data_ptr()
        if self.kind == "sgd" and fused_ok and not self.bf16:
            _lib.check(con.lib.kge_transe_reduce_apply_records_sgd(ctypes.byref(desc), rec.data_ptr(), dst.data_ptr(), n, self.ent,
                                                                   self.rel, rows, counts, n_rows, denom, float(con.alpha),
                                                                   con._stream()), con.lib)
            return
        _lib.check(con.lib.kge_transe_reduce_records(ctypes.byref(desc), rec.data_ptr(), dst.data_ptr(), n, rows, counts, n_rows,
                                                     con._stream()), con.lib)
        self.apply_listed_rows(desc, rows, counts, n_rows, n, denom)

    def advance(self):
        """Once per step, after its last application: lazy Adam's beta powers move on."""
        if self.kind == "lazy_adam":
            self.con._adam_advance()


# ----------------------------------------------------------------------------------------------
# data-parallel layouts
# ----------------------------------------------------------------------------------------------
def setup_flat_buffers(con):
    """Data-parallel layout of the dense path: all tables in ONE flat fp32 buffer cut into world_size equal chunks,
    rank g owning chunk g.  Per step the gradient image is reduce-scattered, the optimizer runs on the owned chunk only
    and the updated chunks are all-gathered (what the reference's ps tasks do for their share of the variables,
    distribute_training.py:193-196).  TransE: the chunk is a whole number of rows of the [(E+R), D] row space, because
    the sign-count update needs whole rows; other models: any 4-element boundary."""
    import torch
    from .parallel import chunk_size
    W = con.world_size
    names = list(con.trainModel.table_names)
    numels = [t.numel() for t in con._tables]
    # PIECES: the flat buffer is cut into K consecutive segments, each of them exchanged and updated like a small data-parallel
    # problem of its own (rank g owns the g-th W-th of every segment), so that the optimizer on piece k and its all-gather run
    # while piece k+1 is still on the wire.  One piece for FB15k-237-sized tables (the exchange is latency-, not size-bound
    # there); four from 64 MB of image on.  `dp_pieces` overrides (tests force 2 on a small graph).
    image_bytes = sum(numels) * 4
    K = int(getattr(con, "dp_pieces", 0)) or (4 if image_bytes >= (64 << 20) else 1)
    if con.use_counts:     # ent_embeddings then rel_embeddings, back to back: rows of one [(E+R), D] space
        D = con.hidden_size
        chunk_rows = chunk_size(con.entTotal + con.relTotal, W, 4 * K)
        if chunk_rows * W == con.entTotal + con.relTotal:
            chunk_rows += 4 * K        # at least one spare row at the end: the loss rides in it (train_step)
        chunk = chunk_rows * D
        offs = [0, numels[0]]
    else:
        offs, off = [], 0
        for n in numels:
            offs.append(off)
            off += -(-n // 64) * 64
        chunk = chunk_size(off + 4, W, 4 * K)     # (+ 4: a spare tail slot for the loss)
    total = chunk * W
    dev = con._tables[0].device
    flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
    flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
    flat_m = torch.zeros(total, dtype=torch.float32, device=dev) if con._adam else None
    flat_v = torch.zeros(total, dtype=torch.float32, device=dev) if con._adam else None
    for i, name in enumerate(names):
        shape = con._tables[i].shape
        view = flat_p[offs[i]:offs[i] + numels[i]].view(shape)
        view.copy_(con._tables[i])
        con._tables[i] = view
        con.trainModel.parameter_lists[name] = view
        setattr(con.trainModel, name, view)
        con._grads[i] = flat_g[offs[i]:offs[i] + numels[i]].view(shape)
        if con._adam:
            for flat, slots in ((flat_m, con._adam_m), (flat_v, con._adam_v)):
                v = flat[offs[i]:offs[i] + numels[i]].view(shape)
                v.copy_(slots[i])
                slots[i] = v
    con._flat_p, con._flat_g, con._flat_m, con._flat_v = flat_p, flat_g, flat_m, flat_v
    con._chunk = chunk
    con._pieces = K
    seg, own = total // K, chunk // K                     # elements per piece, and per (piece, rank)
    # piece k: segment [k*seg, (k+1)*seg) of the flat buffers; this rank's share of it; where that share sits in the owned images
    con._piece_seg = [(k * seg, (k + 1) * seg) for k in range(K)]
    con._piece_own = [(k * seg + con.rank * own, k * seg + (con.rank + 1) * own) for k in range(K)]
    con._own_len = own
    con._grads_own = torch.zeros(chunk, dtype=torch.float32, device=dev)
    con._loss_tail = total - 1                           # spare element (no table reaches it) of the LAST rank's last piece
    # the loss scalar LIVES in that slot: the step's kernels write this rank's partial loss there, the exchange replaces it by
    # the global one (no copy in either direction)
    con._loss = flat_p[con._loss_tail:]
    if con.use_counts:
        rows_total = chunk_rows * W
        seg_r, own_r = rows_total // K, chunk_rows // K
        live = con.entTotal + con.relTotal
        con._counts = torch.zeros((rows_total, con.hidden_size), dtype=torch.int32, device=dev)
        con._counts_own = torch.zeros((chunk_rows, con.hidden_size), dtype=torch.int32, device=dev)
        con._piece_rows = [(min(k * seg_r + con.rank * own_r, live), min(k * seg_r + (con.rank + 1) * own_r, live)) for k in range(K)]
        con._own_rows_len = own_r
    con._opt_state_synced = True
    con._refresh_pointers()


def setup_shards(con):
    """Table-sharded sparse mode (config #5 on N GPUs): rank g keeps the entity rows [g*chunk, (g+1)*chunk) only; the
    relation table stays replicated.  The shard is cut from the table this rank initialised with the common seed, so
    the union of the shards is the single-process table."""
    import torch
    from .parallel import chunk_size
    if con.hidden_size % 4:
        raise KgeError("the table-sharded sparse mode needs an embedding width that is a multiple of 4")
    if con.world_size > 64:
        raise KgeError("the table-sharded sparse mode supports up to 64 ranks")
    W, g, E, D = con.world_size, con.rank, con.entTotal, con.hidden_size
    chunk = chunk_size(E, W)
    lo, hi = min(g * chunk, E), min((g + 1) * chunk, E)
    if getattr(con, "_ent_is_shard", False):     # the model drew this rank's rows only (Config._plan_entity_shard); the moments were made shard-sized
        plan = con._shard_plan
        if (plan["world"], plan["rank"], plan["chunk"]) != (W, g, chunk) or con._tables[0].shape[0] != chunk:
            raise KgeError("the entity table was created as the shard of rank %d of %d, the process group has rank %d of %d"
                           % (plan["rank"], plan["world"], g, W))
        con._shard = dict(chunk=chunk, lo=lo, hi=hi)
        con._refresh_pointers()
        return
    full = con._tables[0]
    shard = torch.zeros((chunk, D), dtype=torch.float32, device=full.device)
    if hi > lo:
        shard[:hi - lo].copy_(full[lo:hi])
    con._tables[0] = shard
    con.trainModel.parameter_lists["ent_embeddings"] = shard
    con.trainModel.ent_embeddings = shard
    del full
    if con._lazy_adam:     # the moments of the entity rows are sharded with them (owner computes); the relation table's stay replicated
        for slots in (con._adam_m, con._adam_v):
            old = slots[0]
            slots[0] = torch.zeros((chunk, D), dtype=torch.float32, device=shard.device)
            if hi > lo:
                slots[0][:hi - lo].copy_(old[lo:hi])
            del old
    if con._adagrad:       # the accumulator of the entity rows likewise (pad rows of the last shard: the initial value, never read)
        old = con._adagrad_acc[0]
        con._adagrad_acc[0] = torch.full((chunk, D), float(con.adagrad_initial_accumulator), dtype=torch.float32, device=shard.device)
        if hi > lo:
            con._adagrad_acc[0][:hi - lo].copy_(old[lo:hi])
        del old
    if con._row_adagrad:   # ... and the per-row accumulators of the entity rows, one float each
        old = con._rowadagrad_acc[0]
        con._rowadagrad_acc[0] = torch.full((chunk,), float(con.adagrad_initial_accumulator), dtype=torch.float32, device=shard.device)
        if hi > lo:
            con._rowadagrad_acc[0][:hi - lo].copy_(old[lo:hi])
        del old
    torch.cuda.empty_cache()
    con._shard = dict(chunk=chunk, lo=lo, hi=hi)
    con._refresh_pointers()


def dp_exchange(con, image, own_image, apply_piece, counts):
    """The data-parallel part of a dense step: reduce-scatter of the gradient image, the optimizer on the owned share,
    all-gather of the updated parameters -- piece by piece (see setup_flat_buffers), every collective asynchronous, so
    that piece k is updated and sent while piece k+1 is still being summed.  The loss needs no collective of its own: it
    is added into a spare tail slot of the image (TransE's int32 count image: as four 16-bit limbs of a 2^-32 fixed-point
    value, kge_loss_to_limbs), summed by the reduce-scatter like everything else, written by its owner -- the last rank --
    into the spare tail slot of the parameter buffer, and reaches every rank with the all-gather."""
    from .parallel import reduce_scatter_sum, all_gather_chunks
    st, W, K = con._stream(), con.world_size, con._pieces
    flat_img, flat_own = image.view(-1), own_image.view(-1)
    per_seg, per_own = flat_img.numel() // K, flat_own.numel() // K
    ride = flat_img.numel() >= 4 and (not counts or con.hidden_size >= 4)
    last = con.rank == W - 1
    nat = stream_rccl(con) if (K == 1 and ride) else None
    con.comm_fence("nat" if nat is not None else "pg")
    if nat is not None:
        # one piece (tables below 64 MB): the two collectives go onto the engine's own stream, in order with its kernels
        # (parallel.StreamRccl) -- no process-group stream, no event hand-offs
        if counts and not getattr(con, "_limbs_from_emit", False):
            _lib.check(con.lib.kge_loss_to_limbs(con._loss.data_ptr(), flat_img[flat_img.numel() - con.hidden_size:].data_ptr(), st), con.lib)
        elif not counts:
            flat_img[-1:].copy_(con._loss)
        nat.reduce_scatter_sum(flat_own, flat_img, st)
        if last:
            if counts:
                _lib.check(con.lib.kge_limbs_to_loss(flat_own[flat_own.numel() - con.hidden_size:].data_ptr(), con._loss.data_ptr(), st), con.lib)
            else:
                con._loss.copy_(flat_own[-1:])
        apply_piece(0)
        (slo, shi), (lo, hi) = con._piece_seg[0], con._piece_own[0]
        nat.all_gather_chunks(con._flat_p[slo:shi], con._flat_p[lo:hi], st)
        image.zero_()
        if con._adam:
            con._adam_advance()
        con.global_step += 1
        return
    if ride:
        if counts and not getattr(con, "_limbs_from_emit", False):     # (a sampled batch: the emit kernel has written the limbs itself)
            _lib.check(con.lib.kge_loss_to_limbs(con._loss.data_ptr(), flat_img[flat_img.numel() - con.hidden_size:].data_ptr(), st), con.lib)
        else:
            flat_img[-1:].copy_(con._loss)
    rs = [reduce_scatter_sum(flat_own[k * per_own:(k + 1) * per_own], flat_img[k * per_seg:(k + 1) * per_seg], con._pg, async_op=True)
          for k in range(K)]
    if not ride:
        from .parallel import allreduce_sum
        allreduce_sum([con._loss], con._pg)
    ag = []
    for k in range(K):
        if rs[k] is not None:
            rs[k].wait()
        if ride and last and k == K - 1:      # the summed loss -> the parameter buffer's tail slot (before the all-gather of this piece)
            if counts:
                _lib.check(con.lib.kge_limbs_to_loss(flat_own[flat_own.numel() - con.hidden_size:].data_ptr(),
                                                     con._flat_p[con._loss_tail:].data_ptr(), st), con.lib)
            else:
                con._loss.copy_(flat_own[-1:])
        apply_piece(k)
        (slo, shi), (lo, hi) = con._piece_seg[k], con._piece_own[k]
        ag.append(all_gather_chunks(con._flat_p[slo:shi], con._flat_p[lo:hi], con._pg, async_op=True))
    image.zero_()
    if con._adam:
        con._adam_advance()
    con.global_step += 1
    for w in ag:
        if w is not None:
            w.wait()
    # (ride: con._loss IS the tail slot of the parameter buffer -- the all-gather has just delivered the global loss into it)


def stream_rccl(con):
    """The communicator for collectives on the engine's stream (parallel.StreamRccl): "nccl" backend, `stream_rccl` not switched
    off (KGE_STREAM_RCCL=0 switches it off from the environment).  Created on first use -- collectively: every rank reaches the
    first data-parallel step together -- and PROBED before it is trusted: a reduce-scatter and an all-gather of known values
    through it must give the known sums on every rank, else (or on any error) all ranks fall back to the process group."""
    if getattr(con, "_nat_rccl", None) is None:
        import torch.distributed as dist
        want = getattr(con, "stream_rccl", os.environ.get("KGE_STREAM_RCCL", "1") != "0") and dist.is_initialized() and \
            dist.get_backend(con._pg) == "nccl"
        nat = False
        if want:
            import sys
            import torch
            from .parallel import StreamRccl
            con.comm_fence("pg")
            good = 0
            try:
                nat = StreamRccl(con._pg)
                torch.cuda.synchronize(con.device)
                W, g, st = nat.world, nat.rank, con._stream()
                src = torch.arange(4 * W, dtype=torch.int32, device=con.device) + g          # rank g contributes i + g
                own = torch.empty(4, dtype=torch.int32, device=con.device)
                nat.reduce_scatter_sum(own, src, st)
                full = torch.empty(4 * W, dtype=torch.int32, device=con.device)
                full[4 * g:4 * g + 4] = own
                nat.all_gather_chunks(full, full[4 * g:4 * g + 4], st)
                torch.cuda.synchronize(con.device)
                want_full = W * torch.arange(4 * W, dtype=torch.int32) + W * (W - 1) // 2      # sum_g (i + g)
                good = int(torch.equal(full.cpu(), want_full))
                if not good:
                    print("StreamRccl probe gave wrong sums: collectives stay on the process group's stream", file=sys.stderr)
            except Exception as exc:       # still RCCL either way: the process-group path is the documented alternative
                print("StreamRccl unavailable (%s): collectives stay on the process group's stream" % exc, file=sys.stderr)
            # every rank must take the same path (a rank on the other communicator would wait for ever): agree on the minimum
            ok = torch.tensor([good], dtype=torch.int32, device=con.device)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=con._pg)
            if int(ok.item()) == 0:
                if nat:
                    nat.close()
                nat = False
        con._nat_rccl = nat
    return con._nat_rccl or None


# ----------------------------------------------------------------------------------------------
# step paths
# ----------------------------------------------------------------------------------------------
def inplace_step(con, dev, n_pos, stride, denom, hand_fed):
    """TransH / TransD (and TransE off the sign-count path) on one rank: forward / backward and the rows rule on the touched rows
    in place from float gradient records -- no gradient tables, no sweep."""
    con._rule.forward_backward_rows(dev, n_pos, con.negative_ent + con.negative_rel, stride, denom)
    con._rule.advance()
    if hand_fed:       # a hand-fed batch may hold negatives the in-place update cannot take (the sampler draws none)
        skipped = ctypes.c_int32(0)
        _lib.check(con.lib.kge_sgd_rows_skipped(ctypes.byref(skipped)), con.lib)
        if skipped.value:
            raise KgeError("sparse_rows: %d negatives are not single-slot corruptions of their positive and were left out "
                           "of this step; train such batches with sparse_rows=False" % skipped.value)
    con.global_step += 1


def counts_step(con, dev, n_pos, stride, denom, sampled, pack, ahead):
    """TransE's sign-count step at a large batch: exact int32 gradient counts, SGD or TF1 Adam on the whole tables; across ranks
    the count image is what is exchanged.  ahead: draw the next batch during this step."""
    if ahead:
        con._attach_next_batch()              # rides in the scatter launch enqueued by forward_counts
    # data-parallel: the emit kernel of a sampled batch also writes the loss as limbs into the count image's spare tail slot
    con._limbs_from_emit = bool(con._dp and sampled and con.hidden_size >= 4)
    target = con._counts.view(-1)[con._counts.numel() - con.hidden_size:].data_ptr() if con._limbs_from_emit else 0
    if target != getattr(con, "_limbs_target", 0):
        con.lib.kge_loss_limbs_target(ctypes.c_void_p(target) if target else None)
        con._limbs_target = target
    # one process: forward, segmented sum and optimizer in ONE call (kge_transe_train_step_counts) -- the rows whose records one
    # team can hold are summed in registers and updated there, without the count image; `fused_counts = False` keeps the
    # two-call form (the data-parallel step needs the image: it is what the ranks exchange)
    one_call = not con._dp and bool(getattr(con, "fused_counts", True))
    try:
        if one_call:
            con.step_counts(dev, n_pos, stride, denom, sampler_shaped=sampled, pack=pack)
        else:
            con.forward_counts(dev, n_pos, stride, denom, sampler_shaped=sampled, pack=pack)
    finally:
        if ahead:                              # launched on its own if the step's path had no scatter kernel -- and
            con._flush_next_batch()           # also when the forward call failed: an armed sampler never outlives its buffers
    if one_call:
        pass
    elif con._dp:
        # int32 SUM is exact: rank g receives the summed counts of ITS rows, updates them, and the updated rows go round
        dp_exchange(con, con._counts, con._counts_own, lambda k: con.apply_counts(denom, own=True, piece=k), counts=True)
        con.tables_changed()
    else:
        con.apply_counts(denom)


def dense_step(con, dev, n_pos, stride, denom, sampled, ahead):
    """The fp32 gradient-table step (every model; TransE at a small batch): forward / backward into the gradient tables, then the
    optimizer on the whole tables -- across ranks on the owned share of the flat buffer.  ahead: draw the next batch during
    this step."""
    # one GPU: the next batch's sampler rides in a launch of the step that leaves most of the chip idle -- TransR's relation
    # scatter, the record paths' bucket scatter, the atomic path's forward/backward kernel itself (a few hundred
    # latency-bound workgroups at the reference's batch sizes); a path without such a launch runs it on its own afterwards
    ride = ahead and not con._dp
    if ride:
        con._attach_next_batch()
    try:
        con.forward_backward(dev, n_pos, stride, denom, sampler_shaped=sampled)
    finally:
        if ride:
            con._flush_next_batch()
    if ahead and not ride:
        con._prefetch_next_batch(behind_emit=bool(con.lib.kge_pair_path_active(ctypes.byref(con._desc), n_pos,
                                                                               con.negative_ent + con.negative_rel)))
    if con._dp:
        dp_exchange(con, con._flat_g, con._grads_own, lambda k: con.apply_gradients(own=True, piece=k), counts=False)
    else:
        con.apply_gradients()


def records_step(con, dev_batch, n_pos, stride, denom):
    """The rows rule in place across ranks (TransH / TransD, or TransE off the sign-count path, with sparse_rows): the tables --
    and with LazyAdam their moments, with Adagrad their accumulators -- are replicated; every rank turns ITS slice of the batch
    into float gradient records, the records (rows + destination keys) are all-gathered -- the sparse touched-row exchange: only
    rows a step touches travel -- and every rank adds -lr * the per-row sums of ALL records to its replica (LazyAdam, Adagrad:
    puts them through the rule on the rows that have a record).  Every rank reduces the same records in the same order, so the
    replicas stay bit-identical; against the single-process step the per-row sums differ in fp32 order only.  Replaces the
    scatter_sub updates the reference's workers send to its parameter servers (distribute_training.py:99-101,193-196)."""
    import torch
    from .parallel import all_gather_chunks, allreduce_sum, max_slice_positions
    n_neg = con.negative_ent + con.negative_rel
    W, D = con.world_size, con.hidden_size
    slots = {_lib.TRANSE: 3 + n_neg, _lib.TRANSH: 4 + n_neg, _lib.TRANSD: 6 + 2 * n_neg}[con.trainModel.model_id]
    b = getattr(con, "_rec_buf", None)
    if b is None or b["slots"] != slots:
        per = max_slice_positions(con.lib, con.batch_size, W, con.workThreads) * slots     # records per rank's slice
        b = dict(slots=slots, per=per,
                 rec=torch.zeros((W * per, D), dtype=torch.float32, device=con.device),
                 dst=torch.full((W * per,), -1, dtype=torch.int32, device=con.device))
        con._rec_buf = b
    per, off = b["per"], con.rank * b["per"]
    _lib.check(con.lib.kge_forward_backward_records(
        ctypes.byref(con._desc), con._tab_ptrs, dev_batch[0].data_ptr(), dev_batch[1].data_ptr(), dev_batch[2].data_ptr(),
        n_pos, n_neg, stride, denom, con.batch_size, b["rec"].data_ptr(), b["dst"].data_ptr(), off, per,
        con._loss.data_ptr(), con._stream()), con.lib)
    if W > 1:
        con.comm_fence("pg")
        all_gather_chunks(b["rec"].view(-1), b["rec"][off:off + per].view(-1), con._pg)
        all_gather_chunks(b["dst"], b["dst"][off:off + per], con._pg)
        allreduce_sum([con._loss], con._pg)
    # (slot tables are replicated like the tables: the same rate and the same records in the same order on every rank)
    con._rule.apply_float_records(b["rec"], b["dst"], W * per, con.batch_size, n_neg)
    con._rule.advance()
    con.global_step += 1


def sparse_step(con, dev_batch, n_pos, stride, denom, check_shape=False):
    """Sparse-row TransE step on ONE GPU: emit int8 records -> sort by destination row -> compact per-row counts ->
    the rows rule on the touched rows.  Bitwise the same update as the dense count image (integer sums).  N GPUs:
    sharded_step."""
    import torch
    n_neg = con.negative_ent + con.negative_rel
    D = con.hidden_size
    m_local = stride * (3 + n_neg)
    dw = int(con.lib.kge_transe_record_dwords(ctypes.byref(con._desc)))
    buf = con._sparse_buf
    if buf is None or buf.get("m_local") != m_local:
        dev = con.device
        buf = dict(m_local=m_local,
                   rec=torch.empty((m_local, dw), dtype=torch.int32, device=dev),
                   dst=torch.empty(m_local, dtype=torch.int32, device=dev),
                   rows=torch.empty(m_local, dtype=torch.int32, device=dev),
                   row_counts=torch.empty((m_local, D), dtype=torch.int32, device=dev),
                   n_rows=torch.zeros(1, dtype=torch.int32, device=dev))
        con._sparse_buf = buf
    st = con._stream()
    buf["dst"].fill_(-1)
    if con._bf16:       # bf16 table storage: its own emit kernel, the same records
        _lib.check(con.lib.kge_transe_emit_records_bf16(
            ctypes.byref(con._desc), con._tables[0].data_ptr(), con._tables[1].data_ptr(),
            dev_batch[0].data_ptr(), dev_batch[1].data_ptr(), dev_batch[2].data_ptr(), n_pos, n_neg,
            dev_batch.shape[1] // (1 + n_neg), denom, buf["rec"].data_ptr(), buf["dst"].data_ptr(), con._loss.data_ptr(), st), con.lib)
    else:
        _lib.check(con.lib.kge_transe_emit_records(
            ctypes.byref(con._desc), con._tables[0].data_ptr(), con._tables[1].data_ptr(),
            dev_batch[0].data_ptr(), dev_batch[1].data_ptr(), dev_batch[2].data_ptr(), n_pos, n_neg,
            dev_batch.shape[1] // (1 + n_neg), denom, buf["rec"].data_ptr(), buf["dst"].data_ptr(), None, None,
            con._loss.data_ptr(), st), con.lib)
    if check_shape:
        nd = ctypes.c_int32(0)
        _lib.check(con.lib.kge_transe_deferred_groups(ctypes.byref(nd)), con.lib)
        if nd.value:
            raise KgeError("sparse_rows: %d groups have negatives that are not single-slot corruptions of their "
                           "positive; train such batches with sparse_rows=False" % nd.value)
    con._rule.reduce_apply(con._desc, buf["rec"], buf["dst"], buf["dst"].numel(), buf, denom,
                           fused_ok=getattr(con, "sparse_fused", True) and D % 4 == 0)
    con._rule.advance()
    con.global_step += 1


def shared_step(con, dev, n_pos, stride, denom):
    """TransE on negatives SHARED by chunks of positives (NON-PARITY, opt-in: Config.set_shared_negatives; the definition is in
    include/kge_mi355.h) on ONE GPU.  `dev` holds the step's positives alone (drawn by the sampler at negRate = 0): the draw
    kernel hashes the chunk's candidates and every pair's side from (seed, global_step) and looks the mask up, the shared emit
    kernel writes 3 n_pos + n_chunks N int8 records in the sparse step's format, and that step's reduce and rows rule finish.
    Buffers only grow."""
    import torch
    P, N, D = con._shared_chunk, con.negative_ent, con.hidden_size
    n_chunks, cap_chunks = -(-n_pos // P), -(-stride // P)
    m_cap = 3 * stride + cap_chunks * N
    buf = con._sparse_buf
    if buf is None or buf.get("shared_cap", 0) < m_cap or buf["pair"].shape[0] < stride:
        d = con.device
        dw = int(con.lib.kge_transe_record_dwords(ctypes.byref(con._desc)))
        buf = dict(shared_cap=m_cap,
                   cand=torch.empty((cap_chunks, N), dtype=torch.int32, device=d),
                   pair=torch.empty((stride, N), dtype=torch.uint8, device=d),
                   rec=torch.empty((m_cap, dw), dtype=torch.int32, device=d),
                   dst=torch.empty(m_cap, dtype=torch.int32, device=d),
                   rows=torch.empty(m_cap, dtype=torch.int32, device=d),
                   row_counts=torch.empty((m_cap, D), dtype=torch.int32, device=d),
                   n_rows=torch.zeros(1, dtype=torch.int32, device=d))
        con._sparse_buf = buf
    st = con._stream()
    h, t, r = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
    _lib.check(con.lib.kge_shared_negatives_draw(h, t, r, n_pos, con._first_pos, P, N, con._shared_seed, con.global_step,
                                                 buf["cand"].data_ptr(), buf["pair"].data_ptr(), st), con.lib)
    # bf16 table storage: the same kernel reading stored bf16 rows, the same records
    emit = con.lib.kge_transe_emit_records_shared_bf16 if con._bf16 else con.lib.kge_transe_emit_records_shared
    _lib.check(emit(ctypes.byref(con._desc), con._tables[0].data_ptr(), con._tables[1].data_ptr(),
                    h, t, r, n_pos, stride, P, buf["cand"].data_ptr(), N, buf["pair"].data_ptr(),
                    denom, buf["rec"].data_ptr(), buf["dst"].data_ptr(), con._loss.data_ptr(), st),
               con.lib)
    buf["shared_step"], buf["shared_shape"], buf["shared_batch"] = con.global_step, (n_pos, n_chunks), dev
    con._rule.reduce_apply(con._desc, buf["rec"], buf["dst"], 3 * n_pos + n_chunks * N, buf, denom,
                           fused_ok=getattr(con, "sparse_fused", True) and D % 4 == 0)
    con._rule.advance()
    con.global_step += 1


def shared_chunk_cap(n_pos, P, rel_total):
    """The bound on the chunks of a relation-grouped batch: ceil(n_pos / P) + min(rel_total + 1, n_pos) (a run's last piece may be
    short, and there are at most rel_total + 1 runs).  kge_shared_chunk_cap's value, for callers without the library."""
    n_pos, P, rel_total = int(n_pos), int(P), int(rel_total)
    if n_pos < 0 or P < 1 or rel_total < 0:
        raise ValueError("shared_chunk_cap: n_pos >= 0, P >= 1 and rel_total >= 0, got %r" % ((n_pos, P, rel_total),))
    return -(-n_pos // P) + min(rel_total + 1, n_pos)


def shared_relation_chunks(r, P, rel_total):
    """(perm int32 [n_pos], chunks int32 [cap, 2], n_chunks): the order and the chunk table of relation-grouped shared negatives,
    in plain numpy -- the one host statement of the definition (include/kge_mi355.h).  perm is the stable order of the batch
    positions by relation id, an id outside [0, rel_total) sorting as rel_total; the run of a relation is cut from its start into
    pieces of P sorted positions, the last may be short; chunks[j] = (first sorted position, length) of piece j, and the slots
    from n_chunks to cap = shared_chunk_cap(n_pos, P, rel_total) are (n_pos, 0)."""
    import numpy as np
    r = np.asarray(r).reshape(-1).astype(np.int64)
    P, rel_total = int(P), int(rel_total)
    n_pos = len(r)
    cap = shared_chunk_cap(n_pos, P, rel_total)
    key = np.where((r >= 0) & (r < rel_total), r, rel_total)
    perm = np.argsort(key, kind="stable").astype(np.int32)
    skey = key[perm]
    starts = np.flatnonzero(np.r_[True, skey[1:] != skey[:-1]]) if n_pos else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], n_pos] if n_pos else starts
    first = np.concatenate([np.arange(a, b, P) for a, b in zip(starts, ends)]) if n_pos else np.zeros(0, dtype=np.int64)
    run_end = np.concatenate([np.full(-(-(b - a) // P), b) for a, b in zip(starts, ends)]) if n_pos else first
    n_chunks = len(first)
    chunks = np.zeros((cap, 2), dtype=np.int32)
    chunks[:, 0] = n_pos
    chunks[:n_chunks, 0] = first
    chunks[:n_chunks, 1] = np.minimum(P, run_end - first)
    return perm, chunks, n_chunks


def _mix64(z):
    """splitmix64's output function on numpy uint64 (csrc/mix_dev.hpp mix64), mod 2^64."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=u)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        return z ^ (z >> u(31))


def shared_in_chunk_candidates(h2, t2, chunks, n_chunks, sides, N, K, seed, step, valid=None):
    """int32 [n_chunks, K]: the in-chunk candidates of relation-grouped shared negatives, in plain numpy -- the one host statement
    of their rotation and ids (include/kge_mi355.h, "In-chunk candidates").  h2 / t2: the positives in sorted order; chunks: the
    table of shared_relation_chunks; sides: [n_chunks, K] for the in-chunk columns, or [n_chunks, N + K] for all (columns N on
    are read), 0 = new tail, 1 = new head -- bit 0 of `pair` at any position of the chunk.  Chunk j = (first, len) is rotated by
    o_j = ((mix(S + (((j << 8) | 64) + 1) G) >> 32) * len) >> 32 with S = mix(seed + (step + 1) G); column N + i is
    t2[first + (o_j + i) % len] for a new tail, h2[...] for a new head, and -1 for i >= len.  valid (bool [n_chunks], optional):
    False where the chunk's relation lies outside the table -- the trailing run, whose K ids are -1."""
    u = np.uint64
    G = 0x9E3779B97F4A7C15
    h2, t2 = np.asarray(h2).reshape(-1), np.asarray(t2).reshape(-1)
    chunks = np.asarray(chunks).reshape(-1, 2)[:int(n_chunks)].astype(np.int64)
    N, K, n_chunks = int(N), int(K), int(n_chunks)
    sides = np.asarray(sides).astype(np.int64)
    sides = sides.reshape(n_chunks, sides.size // n_chunks if n_chunks else K)
    if sides.shape[1] not in (K, N + K):
        raise ValueError("shared_in_chunk_candidates: sides is [n_chunks, K] or [n_chunks, N + K], got %r" % (sides.shape,))
    sides = sides[:, sides.shape[1] - K:] & 1
    S = _mix64(u((int(seed) + (int(step) + 1) * G) & 0xFFFFFFFFFFFFFFFF))
    first, length = chunks[:, 0], chunks[:, 1]
    with np.errstate(over="ignore"):
        key = (np.arange(n_chunks, dtype=u) << u(8)) | u(64)
        o = (((_mix64(S + (key + u(1)) * u(G)) >> u(32)) * length.astype(u)) >> u(32)).astype(np.int64)
    i = np.arange(K, dtype=np.int64)[None, :]
    inside = i < length[:, None]
    if valid is not None:
        inside = inside & np.asarray(valid, dtype=bool).reshape(-1, 1)
    q = np.where(inside, first[:, None] + (o[:, None] + i) % np.maximum(length, 1)[:, None], 0)
    if len(h2) == 0:
        return np.full((n_chunks, K), -1, dtype=np.int32)
    ids = np.where(sides == 0, t2[q], h2[q])
    return np.where(inside, ids, -1).astype(np.int32)


def shared_grouped_draw(con,h2, t2, r2, n_pos, chunks, cap, cand, pair):
    """The draw stage of both grouped steps (device pointers): the N = negative_ent drawn candidates of every chunk slot, and with
    in_chunk = K > 0 the K in-chunk ones beside them, into lists N + K wide.  K = 0 makes the call it always made."""
    L, N, K = con.lib, con.negative_ent, con._shared_in_chunk
    typed = 1 if con.type_constrained_sampling else 0
    if K:
        _lib.check(L.kge_shared_negatives_draw_grouped_mixed(h2, t2, r2, n_pos, chunks, cap, N, K, typed, con._shared_seed, con.global_step,
                                                             cand, pair, con._stream()), L)
    else:
        _lib.check(L.kge_shared_negatives_draw_grouped(h2, t2, r2, n_pos, chunks, cap, N, typed, con._shared_seed, con.global_step,
                                                       cand, pair, con._stream()), L)


def shared_grouped_step(con, dev, n_pos, stride, denom):
    """shared_step on RELATION-GROUPED chunks (Config.set_shared_negatives(..., by_relation=True); NON-PARITY, opt-in; one rank):
    the ordering stage sorts the step's positives by relation and cuts the runs into chunks of at most P, the grouped draw hashes a
    chunk's candidates and their sides from (seed, global_step) -- from the relation's type lists with type-constrained sampling
    on -- and looks the masks up, the emit kernel reads its chunks from the table, and the sparse step's reduce and rows rule
    finish over 3 n_pos + cap N records.  The chunk count stays on the device: everything is sized by cap =
    shared_chunk_cap(stride, P, relTotal), and the step has no host synchronisation.  Buffers only grow.
    TransH (the model is read from the Config): same order, same draw, same buffer names; the chunk's one normal vector and one
    r^ are shared too.  kge_transh_emit_records_shared_chunks writes 2 n_pos + cap (N + 2) FLOAT records -- h and t per position,
    the relation row, the normal vector and N candidates per chunk slot -- keyed in the row space of the unshared TransH step,
    and the rows rule takes them as it takes that step's (RowsRule.apply_float_records).
    TransD: the same again with kge_transd_emit_records_shared_chunks and 4 n_pos + cap (2 N + 2) float records -- every entity
    has a record for its ent_embeddings row and one for its ent_transfer row, the chunk slot one for rel_embeddings and one for
    rel_transfer -- keyed in the row space of the unshared TransD step.
    TransR: same order, same draw, same buffer names, no records: kge_transr_forward_backward_shared_chunks puts the chunk table's
    2 n_pos + cap N rows through the projection, the pair walk, dgrad and wgrad into the dense gradient tables, and
    Config.apply_gradients finishes as it does for the unshared TransR step."""
    import torch
    model_id = con.trainModel.model_id
    if model_id == _lib.TRANSR:
        return shared_grouped_transr_step(con, dev, n_pos, stride, denom)
    # N: the candidate columns of a chunk, drawn and in-chunk (set_shared_negatives(..., in_chunk=K); "In-chunk candidates"): the
    # emit kernels and the rows rule take the wider lists as they take any
    P, N, D = con._shared_chunk, con.negative_ent + con._shared_in_chunk, con.hidden_size
    float_rec = model_id in (_lib.TRANSH, _lib.TRANSD)      # the float-record models
    ew = 2 if model_id == _lib.TRANSD else 1                # records per entity
    cap = shared_chunk_cap(n_pos, P, con.relTotal)
    cap_max = shared_chunk_cap(stride, P, con.relTotal)
    m_cap = 2 * ew * stride + cap_max * (ew * N + 2) if float_rec else 3 * stride + cap_max * N
    buf = con._sparse_buf
    if buf is None or "chunks" not in buf or buf.get("shared_cap", 0) < m_cap or buf["pair"].shape[0] < stride:
        d = con.device
        i32 = torch.int32
        buf = dict(shared_cap=m_cap,
                   perm=torch.empty(stride, dtype=i32, device=d), sorted=torch.empty((3, stride), dtype=i32, device=d),
                   chunks=torch.empty((cap_max, 2), dtype=i32, device=d), n_chunks=torch.zeros(1, dtype=i32, device=d),
                   cand=torch.empty((cap_max, N), dtype=i32, device=d),
                   pair=torch.empty((stride, N), dtype=torch.uint8, device=d),
                   dst=torch.empty(m_cap, dtype=i32, device=d))
        if float_rec:
            buf.update(rec=torch.empty((m_cap, D), dtype=torch.float32, device=d))
        else:
            dw = int(con.lib.kge_transe_record_dwords(ctypes.byref(con._desc)))
            buf.update(rec=torch.empty((m_cap, dw), dtype=i32, device=d),
                       rows=torch.empty(m_cap, dtype=i32, device=d),
                       row_counts=torch.empty((m_cap, D), dtype=i32, device=d),
                       n_rows=torch.zeros(1, dtype=i32, device=d))
        con._sparse_buf = buf
    L, st = con.lib, con._stream()
    h, t, r = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
    h2, t2, r2 = (buf["sorted"][i].data_ptr() for i in range(3))
    chunks, cand, pair = buf["chunks"].data_ptr(), buf["cand"].data_ptr(), buf["pair"].data_ptr()
    _lib.check(L.kge_shared_order_by_relation(h, t, r, n_pos, P, buf["perm"].data_ptr(), h2, t2, r2, chunks, buf["n_chunks"].data_ptr(), st), L)
    shared_grouped_draw(con, h2, t2, r2, n_pos, chunks, cap, cand, pair)
    if float_rec:
        M = 2 * ew * n_pos + cap * (ew * N + 2)
        emit = L.kge_transd_emit_records_shared_chunks if model_id == _lib.TRANSD else L.kge_transh_emit_records_shared_chunks
        _lib.check(emit(ctypes.byref(con._desc), con._tab_ptrs, h2, t2, r2, n_pos, stride, chunks, cap, cand, N, pair, denom, con.batch_size,
                        buf["rec"].data_ptr(), buf["dst"].data_ptr(), con._loss.data_ptr(), st), L)
        buf["shared_step"], buf["shared_shape"], buf["shared_batch"] = con.global_step, (n_pos, cap), dev
        con._rule.apply_float_records(buf["rec"], buf["dst"], M, con.batch_size, N)
        con._rule.advance()
        con.global_step += 1
        return
    emit = L.kge_transe_emit_records_shared_chunks_bf16 if con._bf16 else L.kge_transe_emit_records_shared_chunks      # (bf16 table storage)
    _lib.check(emit(ctypes.byref(con._desc), con._tables[0].data_ptr(), con._tables[1].data_ptr(), h2, t2, r2,
                    n_pos, stride, chunks, cap, cand, N, pair, denom, buf["rec"].data_ptr(),
                    buf["dst"].data_ptr(), con._loss.data_ptr(), st), L)
    buf["shared_step"], buf["shared_shape"], buf["shared_batch"] = con.global_step, (n_pos, cap), dev
    con._rule.reduce_apply(con._desc, buf["rec"], buf["dst"], 3 * n_pos + cap * N, buf, denom,
                           fused_ok=getattr(con, "sparse_fused", True) and D % 4 == 0)
    con._rule.advance()
    con.global_step += 1


def shared_grouped_transr_step(con, dev, n_pos, stride, denom):
    """shared_grouped_step for TransR (one rank): order -> grouped draw -> kge_transr_forward_backward_shared_chunks into the dense
    gradient tables -> the optimizer on the whole tables.  The lists stay in con._sparse_buf under the names the other models use."""
    import torch
    P, N = con._shared_chunk, con.negative_ent + con._shared_in_chunk      # (N: all candidate columns, drawn and in-chunk)
    cap = shared_chunk_cap(n_pos, P, con.relTotal)
    cap_max = shared_chunk_cap(stride, P, con.relTotal)
    buf = con._sparse_buf
    if buf is None or "chunks" not in buf or buf["chunks"].shape[0] < cap_max or buf["pair"].shape[0] < stride:
        d, i32 = con.device, torch.int32
        buf = dict(perm=torch.empty(stride, dtype=i32, device=d), sorted=torch.empty((3, stride), dtype=i32, device=d),
                   chunks=torch.empty((cap_max, 2), dtype=i32, device=d), n_chunks=torch.zeros(1, dtype=i32, device=d),
                   cand=torch.empty((cap_max, N), dtype=i32, device=d), pair=torch.empty((stride, N), dtype=torch.uint8, device=d))
        con._sparse_buf = buf
    L, st = con.lib, con._stream()
    h2, t2, r2 = (buf["sorted"][i].data_ptr() for i in range(3))
    chunks, cand, pair = buf["chunks"].data_ptr(), buf["cand"].data_ptr(), buf["pair"].data_ptr()
    _lib.check(L.kge_shared_order_by_relation(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n_pos, P, buf["perm"].data_ptr(),
                                              h2, t2, r2, chunks, buf["n_chunks"].data_ptr(), st), L)
    shared_grouped_draw(con, h2, t2, r2, n_pos, chunks, cap, cand, pair)
    _lib.check(L.kge_transr_forward_backward_shared_chunks(ctypes.byref(con._desc), con._tab_ptrs, h2, t2, r2, n_pos, stride, chunks, cap, cand,
                                                           N, pair, denom, con._grad_ptrs, con._loss.data_ptr(), st), L)
    buf["shared_step"], buf["shared_shape"], buf["shared_batch"] = con.global_step, (n_pos, cap), dev
    con.apply_gradients()      # (advances global_step)


def shared_chunk_span(first_position, n_pos, P):
    """(c0, n_chunks): the global chunks of P positions that the batch positions [first_position, first_position + n_pos) meet --
    c0 = first_position // P through (first_position + n_pos - 1) // P; the first and the last may be partial; no position, no
    chunk.  The one place the host computes the span (the kernels' form is in include/kge_mi355.h)."""
    first_position, n_pos, P = int(first_position), int(n_pos), int(P)
    if first_position < 0 or n_pos < 0 or P < 1:
        raise ValueError("shared_chunk_span: first_position >= 0, n_pos >= 0 and P >= 1, got %r" % ((first_position, n_pos, P),))
    c0 = first_position // P
    return c0, ((first_position + n_pos - 1) // P - c0 + 1 if n_pos else 0)


def shared_sharded_step(con, dev, n_pos, stride, denom):
    """shared_step on a SHARDED entity table (more than one rank, or the one-rank rehearsal): sharded_step's stages around the
    shared kernels.  `dev` holds this rank's slice of the step's positives -- the batch positions [_first_pos, _first_pos + n_pos),
    which need not begin on a chunk boundary: chunks are chunks of the GLOBAL position, so the draw at _first_pos gives this rank
    the lists one process would hold for them.  A chunk requests its 2 P + N rows (sharded_step: P (2 + N)) and sends back records
    for them alone; the candidate records of a chunk cut by a slice bound come from both ranks and meet at the row's owner.
    M = 3 n_pos + n_chunks N records; `denom` is the global batch_size * N.  Integer sums, hashes of the global position: the
    union of the shards equals the one-process shared step bit for bit.  An empty slice still joins every collective."""
    import torch
    L, st = con.lib, con._stream()
    con.comm_fence("pg")
    P, N, first = con._shared_chunk, con.negative_ent, con._first_pos
    n_chunks = shared_chunk_span(first, n_pos, P)[1]
    cap_chunks = max(shared_chunk_span(first, stride, P)[1], 1)
    n_cand = n_chunks * N
    M = 3 * n_pos + n_cand
    b = shard_buffers(con, M, 0, 0)
    if "pair" not in b or b["pair"].shape[0] < stride or b["cand"].shape != (cap_chunks, N):
        d = con.device
        b.update(cand=torch.empty((cap_chunks, N), dtype=torch.int32, device=d), cand2=torch.empty((cap_chunks, N), dtype=torch.int32, device=d),
                 pair=torch.empty((stride, N), dtype=torch.uint8, device=d), ht2=torch.empty((2, stride), dtype=torch.int32, device=d))
    h, t, r = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
    cand, cand2, pair, h2, t2 = b["cand"].data_ptr(), b["cand2"].data_ptr(), b["pair"].data_ptr(), b["ht2"][0].data_ptr(), b["ht2"][1].data_ptr()
    _lib.check(L.kge_shared_negatives_draw_at(h, t, r, n_pos, first, P, N, con._shared_seed, con.global_step, cand, pair, st), L)
    # the rows of the positives and of the chunks' candidates, once per chunk
    _lib.check(L.kge_shard_requests_shared(h, t, n_pos, cand, n_cand, con.entTotal, b["req"].data_ptr(), st), L)
    b, n_send, n_recv = shard_fetch_rows(con, M, 2 * n_pos + n_cand)
    _lib.check(L.kge_shard_remap_shared(h, t, n_pos, cand, n_cand, b["slot_of"].data_ptr(), h2, t2, cand2, st), L)
    desc2 = con._desc_with(ent_total=max(n_send, 1))
    _lib.check(L.kge_transe_emit_records_shared_at(ctypes.byref(desc2), b["cache"].data_ptr(), con._tables[1].data_ptr(), h2, t2, r, n_pos,
                                                   stride, first, P, cand2, N, pair, denom, b["rec"].data_ptr(), b["dst"].data_ptr(),
                                                   con._loss.data_ptr(), st), L)
    b["shared_step"], b["shared_shape"], b["shared_batch"] = con.global_step, (n_pos, n_chunks), dev
    shard_finish(con, b, M, n_pos, n_send, n_recv, desc2, denom)


def shard_buffers(con, M, n_recv_rows, n_recv_rec):
    """Workspace of the sharded step, grown geometrically (receive sizes vary from step to step)."""
    import torch
    D, W, dev = con.hidden_size, con.world_size, con.device
    dw = int(con.lib.kge_transe_record_dwords(ctypes.byref(con._desc)))
    b = con._sparse_buf if isinstance(con._sparse_buf, dict) and con._sparse_buf.get("sharded") else dict(sharded=True, M=0, rr=0, rc=0)
    i32 = torch.int32
    if M > b["M"] or "req" not in b:
        cap = max(int(M * 1.25), 64)
        b.update(M=cap, req=torch.empty(cap, dtype=i32, device=dev), slot_of=torch.empty(cap, dtype=i32, device=dev),
                 send_ids=torch.empty(cap, dtype=i32, device=dev), cache=torch.empty((cap, D), dtype=torch.float32, device=dev),
                 rec=torch.empty((cap, dw), dtype=i32, device=dev), dst=torch.empty(cap, dtype=i32, device=dev),
                 ids2=torch.empty(cap, dtype=i32, device=dev), slot_of2=torch.empty(cap, dtype=i32, device=dev),
                 send_rows2=torch.empty(cap, dtype=i32, device=dev), send_rec=torch.empty((cap, dw), dtype=i32, device=dev),
                 counts=torch.zeros(W, dtype=i32, device=dev), cursor=torch.zeros(W, dtype=i32, device=dev),
                 rel_counts=torch.zeros((con.relTotal, D), dtype=i32, device=dev),
                 rel_rows=torch.arange(con.entTotal, con.entTotal + con.relTotal, dtype=i32, device=dev),
                 n_rel=torch.full((1,), con.relTotal, dtype=i32, device=dev), n_rows=torch.zeros(1, dtype=i32, device=dev), dw=dw)
    if n_recv_rows > b["rr"] or "recv_ids" not in b:       # (also for an owner that is never asked for a row: an empty shard)
        cap = max(int(n_recv_rows * 1.25), 64)
        b.update(rr=cap, recv_ids=torch.empty(cap, dtype=i32, device=dev), rows_out=torch.empty((cap, D), dtype=torch.float32, device=dev))
    if n_recv_rec > b["rc"] or "recv_rec" not in b:
        cap = max(int(n_recv_rec * 1.25), 64)
        b.update(rc=cap, recv_rows2=torch.empty(cap, dtype=i32, device=dev), recv_rec=torch.empty((cap, dw), dtype=i32, device=dev),
                 rows=torch.empty(cap, dtype=i32, device=dev), row_counts=torch.empty((cap, D), dtype=i32, device=dev))
    con._sparse_buf = b
    return b


def shard_fetch_rows(con, M, n_req):
    """Both sharded steps, after their request list (b["req"][:n_req], ids < 0 = nothing to fetch) is written: who owns the rows,
    ids out, rows back into b["cache"]; b["slot_of"][i] is request i's row of the cache, b["send_ids"] the cache rows' entity ids.
    `M`: the step's number of records (the workspace is sized by it; n_req <= M).  -> (workspace, rows fetched, rows served)"""
    L, st, W, D, pg = con.lib, con._stream(), con.world_size, con.hidden_size, con._pg
    sh = con._shard
    chunk = sh["chunk"]
    b = shard_buffers(con, M, 0, 0)
    _lib.check(L.kge_shard_count(b["req"].data_ptr(), n_req, chunk, W, b["counts"].data_ptr(), st), L)
    send, recv, gmax = par.exchange_counts_max(b["counts"], pg)
    h_counts = (ctypes.c_int64 * W)(*send)
    _lib.check(L.kge_shard_scatter(b["req"].data_ptr(), n_req, chunk, W, h_counts, b["cursor"].data_ptr(), b["send_ids"].data_ptr(),
                                   b["slot_of"].data_ptr(), st), L)
    n_send, n_recv = sum(send), sum(recv)
    b = shard_buffers(con, M, n_recv, 0)
    # ids out, rows back
    par.all_to_all_rows(b["recv_ids"], b["send_ids"], recv, send, pg, max_rows=gmax)
    _lib.check(L.kge_shard_gather_rows(con._tables[0].data_ptr(), b["recv_ids"].data_ptr(), n_recv, sh["lo"], chunk, D,
                                       b["rows_out"].data_ptr(), st), L)
    par.all_to_all_rows(b["cache"], b["rows_out"], send, recv, pg, max_rows=gmax)
    return b, n_send, n_recv


def sharded_step(con, dev_batch, n_pos, stride, denom):
    """Sparse-row TransE step on a SHARDED entity table (world_size > 1): every stage is O(local batch).
    request ids -> all-to-all -> owners gather rows -> all-to-all -> emit int8 records against the fetched rows ->
    all-to-all (row id, record) -> owners sort / sum / apply their rows; relation counts all-reduced (csrc/shard.hip).
    Integer sums and one per-row update formula: the union of the shards equals the single-process table bit for bit."""
    import torch
    L, st = con.lib, con._stream()
    con.comm_fence("pg")
    n_neg = con.negative_ent + con.negative_rel
    M = n_pos * (3 + n_neg)
    b = shard_buffers(con, M, 0, 0)
    h, t, r = dev_batch[0], dev_batch[1], dev_batch[2]
    bstride = dev_batch.shape[1] // (1 + n_neg)
    # 1. which entity rows does this slice touch, and who owns them; 2. ids out, rows back
    _lib.check(L.kge_shard_requests(h.data_ptr(), t.data_ptr(), r.data_ptr(), n_pos, n_neg, bstride, b["req"].data_ptr(), st), L)
    b, n_send, n_recv = shard_fetch_rows(con, M, M)
    # 3. the unchanged emit kernel over the fetched rows: the batch in terms of cache slots
    if con._dev_batch2 is None or con._dev_batch2.shape != dev_batch.shape:
        con._dev_batch2 = torch.zeros_like(dev_batch)
    h2, t2 = con._dev_batch2[0], con._dev_batch2[1]
    _lib.check(L.kge_shard_remap_batch(h.data_ptr(), t.data_ptr(), n_pos, n_neg, bstride, b["slot_of"].data_ptr(), h2.data_ptr(),
                                       t2.data_ptr(), st), L)
    desc2 = con._desc_with(ent_total=max(n_send, 1))
    _lib.check(L.kge_transe_emit_records(ctypes.byref(desc2), b["cache"].data_ptr(), con._tables[1].data_ptr(), h2.data_ptr(),
                                         t2.data_ptr(), r.data_ptr(), n_pos, n_neg, bstride, denom, b["rec"].data_ptr(),
                                         b["dst"].data_ptr(), None, None, con._loss.data_ptr(), st), L)
    shard_finish(con, b, M, n_pos, n_send, n_recv, desc2, denom)


def shard_finish(con, b, M, n_pos, n_send, n_recv, desc2, denom):
    """Both sharded steps, after the emit kernel: the M records in b["rec"] / b["dst"] (keys: rows of the fetched-row cache, then
    desc2.ent_total + relation; the relation slots of the positives are records [2 n_pos, 3 n_pos)) -> relation counts
    all-reduced with the loss, entity records to their owners, the rows rule on the owned rows and on the replicated relation
    table; the step ends here (advance, global_step)."""
    import torch
    L, st, W, D, pg = con.lib, con._stream(), con.world_size, con.hidden_size, con._pg
    sh = con._shard
    chunk = sh["chunk"]
    dw = b["dw"]
    # 4. relation rows: dense int32 image, all-reduced (the relation table is replicated)
    b["rel_counts"].zero_()
    rel_live = None
    if con._lazy_adam:
        # which relations have a record on THIS rank -- the relation-slot destinations of its active groups and, with relation
        # negatives, the destinations of its active relation-corrupted negatives (slots 3 + k; a relation may take records from
        # those alone, and one process moves its row then) -- read before the reduce below rewrites the destination keys in place;
        # summed over the ranks with the counts.  Entry R collects everything else (no record, or a fetched-row slot).
        # Stage 7 updates only the relations SOME rank had a record for: a record-less row keeps its value and moments under the
        # lazy rule.  (Adagrad needs no mask: a relation whose all-reduced counts are zero has zero gradient, and the rule leaves
        # it alone.)
        if "rel_live" not in b:
            b["rel_live"] = torch.zeros(con.relTotal + 1, dtype=torch.int32, device=con.device)
        rel_live = b["rel_live"]
        rel_live.zero_()
        if n_pos > 0:
            d = b["dst"][2 * n_pos:(M if con.negative_rel > 0 else 3 * n_pos)]
            idx = torch.where(d >= int(desc2.ent_total), d - int(desc2.ent_total), torch.full_like(d, con.relTotal))
            rel_live.index_fill_(0, idx.long(), 1)
    if D % 4 == 0 and con.negative_rel == 0 and n_pos > 0:
        # the relation-side records are slot 2 of every group -- records [2 n_pos, 3 n_pos): ordered by relation, summed by
        # segments into <= R compact rows, scattered into the image (per-element atomics took 0.4 ms of a 3 ms step)
        cap = min(n_pos, con.relTotal) + 8
        if b.get("relc_cap", 0) < cap:
            b.update(relc_cap=cap, relc_rows=torch.empty(cap, dtype=torch.int32, device=con.device),
                     relc_counts=torch.empty((cap, D), dtype=torch.int32, device=con.device))
        _lib.check(L.kge_transe_reduce_records(ctypes.byref(desc2), b["rec"][2 * n_pos:3 * n_pos].data_ptr(),
                                               b["dst"][2 * n_pos:3 * n_pos].data_ptr(), n_pos, b["relc_rows"].data_ptr(),
                                               b["relc_counts"].data_ptr(), b["n_rows"].data_ptr(), st), L)
        _lib.check(L.kge_shard_scatter_count_rows(b["relc_rows"].data_ptr(), b["relc_counts"].data_ptr(), b["n_rows"].data_ptr(),
                                                  cap, desc2.ent_total, con.relTotal, D, b["rel_counts"].data_ptr(), st), L)
    else:
        _lib.check(L.kge_shard_relation_counts(b["rec"].data_ptr(), b["dst"].data_ptr(), M, desc2.ent_total, con.relTotal, dw, D,
                                               b["rel_counts"].data_ptr(), st), L)
    par.allreduce_sum([b["rel_counts"], con._loss] + ([rel_live] if rel_live is not None else []), pg)
    # 5. entity records to their owners
    _lib.check(L.kge_shard_record_ids(b["dst"].data_ptr(), M, n_send, b["send_ids"].data_ptr(), b["ids2"].data_ptr(), st), L)
    _lib.check(L.kge_shard_count(b["ids2"].data_ptr(), M, chunk, W, b["counts"].data_ptr(), st), L)
    send2, recv2, gmax2 = par.exchange_counts_max(b["counts"], pg)
    h_counts2 = (ctypes.c_int64 * W)(*send2)
    _lib.check(L.kge_shard_scatter(b["ids2"].data_ptr(), M, chunk, W, h_counts2, b["cursor"].data_ptr(), b["send_rows2"].data_ptr(),
                                   b["slot_of2"].data_ptr(), st), L)
    _lib.check(L.kge_shard_pack_records(b["rec"].data_ptr(), b["slot_of2"].data_ptr(), M, dw, b["send_rec"].data_ptr(), st), L)
    n_recv2 = sum(recv2)
    con._exchange_sizes = dict(rows_requested=n_send, rows_served=n_recv, records_sent=sum(send2), records_received=n_recv2)
    b = shard_buffers(con, M, n_recv, n_recv2)
    par.all_to_all_rows(b["recv_rows2"], b["send_rows2"], recv2, send2, pg, max_rows=gmax2)
    par.all_to_all_rows(b["recv_rec"], b["send_rec"], recv2, send2, pg, max_rows=gmax2)
    # 6. owner: sort by row, segmented sum, the rows rule on the touched rows of the shard (and the shard's own slot rows)
    if n_recv2 > 0:
        b["recv_rows2"][:n_recv2].sub_(sh["lo"])
        desc3 = con._desc_with(ent_total=chunk, rel_total=0)
        con._rule.reduce_apply(desc3, b["recv_rec"], b["recv_rows2"], n_recv2, b, denom, fused_ok=True)
    # 7. every rank applies the identical relation update from the all-reduced counts
    con._rule.apply_listed_rows(con._desc, b["rel_rows"].data_ptr(), b["rel_counts"].data_ptr(), b["n_rel"].data_ptr(),
                                con.relTotal, denom, live=rel_live)
    con._rule.advance()
    con.global_step += 1
