"""Shared by the GPU tests of "Evaluation on bf16 tables" (include/kge_mi355.h): stored bf16 tables and their widened fp32 twins
on the device, and the two pairs of entry points called through the C ABI into pre-filled buffers.  No Config is involved: the
entry points take a descriptor and addresses."""
import ctypes

import numpy as np

import bf16_ref as ref

KGE_ERR_NO_DATASET, KGE_ERR_BAD_ARG, KGE_ERR_UNSUPPORTED = -2, -3, -4
FILTERED, DRAWN, TYPED, NO_HEAD = 1, 2, 4, 8
MULTIPLE_OF_8_PER_RUNG = (16, 24, 64, 104, 200, 264, 1024)          # the seven rungs of csrc/team_shape.hpp
FILL = -9


def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


def desc(E, R, De, Dr=None, model=0):
    from openkeonspark_amd import _lib
    return _lib.ModelDesc(model, 0, int(E), int(R), int(De), int(De if Dr is None else Dr), 1.0, 0)


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


class Tables:
    """fp32 tables that ARE bf16 values (the caller rounds or asserts), as stored bits and as widened floats, both on the device."""

    def __init__(self, ent, rel):
        self.ent32, self.rel32 = np.ascontiguousarray(ent, np.float32), np.ascontiguousarray(rel, np.float32)
        bits = [ref.to_bf16(x) for x in (self.ent32, self.rel32)]
        for b, x in zip(bits, (self.ent32, self.rel32)):
            assert np.array_equal(ref.widen(b).view(np.uint32), x.view(np.uint32)), "not bf16 values"
        self.ent_b, self.rel_b = (dev(b.view(np.int16)) for b in bits)
        self.ent_f, self.rel_f = dev(self.ent32), dev(self.rel32)
        self.E, self.D, self.R = self.ent32.shape[0], self.ent32.shape[1], self.rel32.shape[0]
        self.desc = desc(self.E, self.R, self.D)

    @classmethod
    def rounded(cls, ent, rel):
        return cls(ref.widen(ref.to_bf16(ent)), ref.widen(ref.to_bf16(rel)))

    def fp32_ptrs(self):
        from openkeonspark_amd import _lib
        return _lib.table_ptrs([self.ent_f.data_ptr(), self.rel_f.data_ptr()])


def ptr(x):
    return None if x is None else x.data_ptr()


def predict(tabs, h, t, r, bf16=True, d=None, ent=Ellipsis, rel=Ellipsis, n=None):
    """kge_predict_bf16 on the stored tables (bf16) or kge_predict on the widened ones -> (return code, the pre-filled buffer)."""
    import torch
    L = lib()
    ids = dev(np.stack([h, t, r]).reshape(3, -1), np.int32) if len(h) else torch.zeros((3, 1), dtype=torch.int32, device="cuda")
    out = torch.full((max(len(h), 1),), float(FILL), dtype=torch.float32, device="cuda")
    d = tabs.desc if d is None else d
    n = len(h) if n is None else n
    if bf16:
        rc = L.kge_predict_bf16(ctypes.byref(d), ptr(tabs.ent_b if ent is Ellipsis else ent), ptr(tabs.rel_b if rel is Ellipsis else rel),
                                ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n, out.data_ptr(), None)
    else:
        rc = L.kge_predict(ctypes.byref(d), tabs.fp32_ptrs(), ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n, out.data_ptr(), None)
    torch.cuda.synchronize()
    L.kge_clear_error()
    return rc, out.cpu().numpy()      # (one spare element when there are no triples: an empty tensor has no address)


def rank_candidates(tabs, h, t, r, tail, tail_stride, head, head_stride, n_cand, flags, seed=0, bf16=True, d=None, ent=Ellipsis,
                    rel=Ellipsis, n=None, counts=None):
    """kge_rank_candidates_bf16 / kge_rank_candidates; h, t, r, tail, head are device tensors (or None) -> (return code, counts
    int64 numpy [n, 2, 2] from a buffer pre-filled with FILL)."""
    import torch
    L = lib()
    n = len(h) if n is None else n
    if counts is None:
        counts = torch.full((max(len(h), 1), 2, 2), FILL, dtype=torch.int64, device="cuda")
    d = tabs.desc if d is None else d
    tail_args = (ptr(h), ptr(t), ptr(r), n, ptr(tail), tail_stride, ptr(head), head_stride, n_cand, flags, seed, ptr(counts), None)
    if bf16:
        rc = L.kge_rank_candidates_bf16(ctypes.byref(d), ptr(tabs.ent_b if ent is Ellipsis else ent),
                                        ptr(tabs.rel_b if rel is Ellipsis else rel), *tail_args)
    else:
        rc = L.kge_rank_candidates(ctypes.byref(d), tabs.fp32_ptrs(), *tail_args)
    torch.cuda.synchronize()
    L.kge_clear_error()
    return rc, counts.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
