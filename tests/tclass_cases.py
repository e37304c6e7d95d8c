"""Shared by test_tclass_host.py and test_gpu_tclass.py: validation / test lists of chosen per-relation sizes written as a
dataset directory, score sets aimed at the grid search's boundaries, and a NumPy restatement of the device algorithm
(csrc/tclass.hip) -- bin every score once, prefix sum, arg-max under the host's float tie rule."""
import ctypes
import os

import numpy as np

from openkeonspark_amd import _lib
from openkeonspark_amd.Config import Config

F32 = np.float32
INTERVAL = F32(0.01)
LDS_BINS = 16000          # tclass.hip kLdsBins: a relation with n_interval + 2 above this takes the global histogram
FUSED_MAX_TRIPLES = 4096  # tclass.hip kFusedMaxTriples

# relation -> (validation triples, test triples).  r0: the skewed relation (25 chunks of the device's 2048) beside relations of
# 1, 2 and 3 triples; r5 only in validation, r6 only in test; r7 min == max; r8 a grid wider than the LDS histogram.
SHAPES = [(50000, 100), (1, 4), (2, 1), (3, 7), (3000, 500), (40, 0), (0, 50), (5, 9), (60, 80), (200, 150), (4097, 30)]
# relation -> (low, high) of its validation scores
RANGES = {0: (0.25, 8.5), 1: (1.0, 2.0), 2: (-3.0, -1.0), 3: (0.0, 0.5), 4: (-12.0, 19.0), 5: (2.0, 2.5), 6: (0.0, 1.0),
          7: (3.25, 3.25), 8: (-150.0, 260.0), 9: (-4.0, 3.0), 10: (5.0, 40.0)}


def fma32(i, mn):
    """fmaf((float)i, 0.01f, mn) with ONE rounding, for integer arrays i < 2^24 and a float32 mn.  The product is exact in
    double (24 x 24 bits); the sum is rounded to odd in double (TwoSum gives the exact error), and 53 >= 2 * 24 + 2 bits make
    the final rounding to float32 the correctly rounded one."""
    p = np.asarray(i, np.float64) * np.float64(INTERVAL)
    b = np.float64(mn)
    s = p + b
    bb = s - p
    err = (p - (s - bb)) + (b - bb)
    toward = np.where(err > 0, np.inf, -np.inf)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(F32)


def bins_of(s, mn, n):
    """k(s) = min{ i in [0, n] : s <= g(i) }, n + 1 when s > g(n): estimate from the quotient, then exact steps both ways."""
    s = np.asarray(s, F32)
    q = ((s - F32(mn)) / INTERVAL).astype(F32)
    e = np.clip(np.where(q >= F32(n + 1), n + 1, np.maximum(q, 0).astype(np.int64)), 0, n + 1)
    while True:
        down = (e > 0) & (s <= fma32(np.maximum(e - 1, 0), mn))
        if not down.any():
            break
        e = e - down
    while True:
        up = (e <= n) & (s > fma32(np.minimum(e, n), mn))
        if not up.any():
            break
        e = e + up
    return e


def numpy_fit(rel, pos, neg, thresh):
    """getBestThreshold restated as the device computes it; `rel` = the relation of every position of the sorted validation
    list.  Writes thresh[r] for the relations present and returns {r: n_interval}."""
    n_interval = {}
    for r in np.unique(rel):
        m = rel == r
        p, q = pos[m], neg[m]
        mn, mx = min(p.min(), q.min()), max(p.max(), q.max())
        n = int(F32(F32(mx - mn) / INTERVAL))
        n_interval[int(r)] = n
        delta = np.zeros(n + 2, np.int64)
        np.add.at(delta, bins_of(p, mn, n), 1)
        np.add.at(delta, bins_of(q, mn, n), -1)
        correct = len(p) + np.cumsum(delta[:n + 1])
        acc = (1.0 * correct / (2 * len(p))).astype(F32)      # the host compares this float, not the integer
        thresh[r] = fma32(np.array([int(np.argmax(acc))]), mn)[0]   # argmax: the lowest index of the maximum
    return n_interval


def write_lists_dir(path, shapes=SHAPES, entities=64, seed=5):
    """A dataset directory whose validation / test list holds shapes[r][0] / shapes[r][1] triples of relation r."""
    rng = np.random.default_rng(seed)
    R = len(shapes)
    os.makedirs(path, exist_ok=True)
    for name, n in (("entity2id.txt", entities), ("relation2id.txt", R)):
        with open(os.path.join(path, name), "w") as f:
            f.write("%d\n" % n + "".join("x%d\t%d\n" % (i, i) for i in range(n)))
    for name, col in (("train2id.txt", None), ("valid2id.txt", 0), ("test2id.txt", 1)):
        rel = np.arange(R) if col is None else np.repeat(np.arange(R), [s[col] for s in shapes])
        rel = rng.permutation(rel)
        arr = np.stack([rng.integers(0, entities, len(rel)), rng.integers(0, entities, len(rel)), rel], axis=1)
        with open(os.path.join(path, name), "w") as f:
            f.write("%d\n" % len(rel))
            np.savetxt(f, arr, fmt="%d")
    return path if path.endswith("/") else path + "/"


def boundary_scores(rng, n, lo, hi, mn):
    """n float32 scores in [lo, hi]: a third random, the rest ON grid points g(i) = fma(i, 0.01, mn) and one ulp to either side."""
    lo, hi = F32(lo), F32(hi)
    s = rng.uniform(lo, hi, n).astype(F32)
    n_grid = int(F32(F32(hi - mn) / INTERVAL))
    if n_grid >= 1 and n >= 3:
        i = rng.integers(1, n_grid + 1, n)
        g = fma32(i, mn)
        kind = rng.integers(0, 4, n)
        s = np.where(kind == 1, g, s)
        s = np.where(kind == 2, np.nextafter(g, F32(np.inf)), s)
        s = np.where(kind == 3, np.nextafter(g, F32(-np.inf)), s)
        s = np.clip(s, lo, hi).astype(F32)
    return s


def adversarial_scores(shapes=SHAPES, ranges=RANGES, seed=0):
    """(vpos, vneg, tpos, tneg) in the order of the sorted lists (relation-major, as importTestFiles sorts them)."""
    rng = np.random.default_rng(seed)
    out = [[], [], [], []]
    for r, (nv, nt) in enumerate(shapes):
        lo, hi = ranges[r]
        mn = F32(lo)
        vp, vn = boundary_scores(rng, nv, lo, hi, mn), boundary_scores(rng, nv, lo, hi, mn)
        if nv:
            vp[rng.integers(0, nv)] = mn          # the minimum is exactly `lo` (the grid's origin) ...
            vn[rng.integers(0, nv)] = F32(hi)     # ... and the maximum exactly `hi`
        if nv >= 2:   # positives mostly low, negatives mostly high: the best threshold lies inside (the union keeps its min / max)
            swap = (vp > vn) & (rng.random(nv) < 0.8)
            vp[swap], vn[swap] = vn[swap], vp[swap]
        span = F32(hi) - F32(lo)
        tp = boundary_scores(rng, nt, F32(lo) - span / 4, F32(hi) + span / 4 + F32(0.02), mn)
        tn = boundary_scores(rng, nt, F32(lo) - span / 4, F32(hi) + span / 4 + F32(0.02), mn)
        for dst, a in zip(out, (vp, vn, tp, tn)):
            dst.append(a)
    return tuple(np.ascontiguousarray(np.concatenate(a), dtype=F32) for a in out)


def sorted_relations(shapes=SHAPES):
    """The relation of every position of the sorted validation and test lists."""
    return (np.repeat(np.arange(len(shapes)), [s[0] for s in shapes]), np.repeat(np.arange(len(shapes)), [s[1] for s in shapes]))


def declare(L):
    L.get_n_interval.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.get_n_interval.restype = ctypes.c_int64


def open_lists(path, work_threads=1):
    """Config on the directory with the evaluation lists imported -> (lib, con, V, T, R)."""
    L = _lib.lib()
    con = Config()
    con.set_in_path(path)
    con.set_work_threads(work_threads)
    con.init()
    L.kge_clear_error()
    L.importTestFiles()
    _lib.raise_if_error(L)
    declare(L)
    return L, con, L.getValidTotal(), L.getTestTotal(), con.relTotal


def host_fit(L, R, vpos, vneg, fill=-1.0):
    thresh = np.full(R, fill, F32)
    L.getBestThreshold(thresh.ctypes.data, vpos.ctypes.data, vneg.ctypes.data)
    _lib.raise_if_error(L)
    return thresh


def host_counts(thresh, valid_rel, test_rel, tpos, tneg):
    """TP, TN, FP, FN restated in NumPy from Test.h:353-365 (the host routine itself returns only the accuracy, which the
    tests compare separately): relations without validation triples left out, positive right when score <= threshold."""
    keep = np.isin(test_rel, np.unique(valid_rel))
    th = thresh[test_rel]
    tp = int(((tpos <= th) & keep).sum()); tn = int(((tneg > th) & keep).sum())
    return tp, tn, int(keep.sum()) - tn, int(keep.sum()) - tp
