"""Shared by test_roc_host.py and test_gpu_roc.py: validation / test lists whose per-relation sizes put every path and boundary
of kge_tc_roc (csrc/tclass.hip) to work, a NumPy restatement of the device algorithm -- bin every split score
once on the validation grid, cumulative sums, the integer area -- and the library's host get_TPFP as the reference."""
import ctypes

import numpy as np

import tclass_cases as tc

# relation -> (validation triples, test triples).  r0: test-heavy, 25 chunks of the device's 2048 on the global path; r3: min ==
# max, one grid point; r4: exactly 4096 test triples, the last size of the LDS path; r5 only in validation (zeros, AUC NaN); r6
# only in test (empty slice); r7: a 41 001-point grid, wider than the LDS histogram, and 4097 triples; r8: validation-heavy;
# r10: a grid that fits the LDS histogram with more than 4096 test triples.
SHAPES = [(300, 50000), (1, 4), (2, 1), (5, 9), (3000, 4096), (40, 0), (0, 50), (60, 4097), (50000, 100), (200, 150), (10, 6000)]
RANGES = {0: (0.25, 8.5), 1: (1.0, 2.0), 2: (-3.0, -1.0), 3: (3.25, 3.25), 4: (-12.0, 19.0), 5: (2.0, 2.5), 6: (0.0, 1.0),
          7: (-150.0, 260.0), 8: (0.25, 8.5), 9: (-4.0, 3.0), 10: (5.0, 40.0)}
TEST_TOTAL = 64507


def write_lists_dir(path):
    return tc.write_lists_dir(path, shapes=SHAPES)


def adversarial_scores(seed):
    return tc.adversarial_scores(shapes=SHAPES, ranges=RANGES, seed=seed)


def sorted_relations():
    return tc.sorted_relations(SHAPES)


def area2_of(hpos, hneg):
    """sum_k hneg[k] * (2 * TPexcl[k] + hpos[k]) in Python integers."""
    total, before = 0, 0
    for a, b in zip(hpos.tolist(), hneg.tolist()):
        total += b * (2 * before + a)
        before += a
    return total


def numpy_roc(valid_rel, vpos, vneg, split_rel, pos, neg):
    """kge_tc_roc restated: {r: (TP [n + 1], FP [n + 1], area2, n_r, n_interval)} for every relation with validation triples."""
    out = {}
    for r in np.unique(valid_rel):
        m = valid_rel == r
        mn, mx = min(vpos[m].min(), vneg[m].min()), max(vpos[m].max(), vneg[m].max())
        mn = mn + tc.F32(0.0)
        n = int(tc.F32(tc.F32(mx - mn) / tc.INTERVAL))
        s = split_rel == r
        hpos = np.bincount(tc.bins_of(pos[s], mn, n), minlength=n + 2).astype(np.int64)
        hneg = np.bincount(tc.bins_of(neg[s], mn, n), minlength=n + 2).astype(np.int64)
        n_r = int(s.sum())
        out[int(r)] = (np.cumsum(hpos)[:n + 1], np.cumsum(hneg)[:n + 1], area2_of(hpos, hneg) if n_r else 0, n_r, n)
    return out


def trapezoid2(tp, fp, n_r):
    """Twice the area under (0,0), (FP(i),TP(i))..., (n_r,n_r) from the explicit point list, in Python integers."""
    xs = [0] + [int(v) for v in fp] + [n_r]
    ys = [0] + [int(v) for v in tp] + [n_r]
    return sum((xs[i + 1] - xs[i]) * (ys[i + 1] + ys[i]) for i in range(len(xs) - 1))


def declare(L):
    tc.declare(L)
    vp = ctypes.c_void_p
    L.get_TPFP.argtypes = [ctypes.c_int64, vp, vp, vp, vp]
    L.get_TPFP.restype = ctypes.POINTER(ctypes.c_int64)


def host_tpfp(L, r, vpos, vneg, tpos, tneg):
    """The library's host get_TPFP(r) as one int64 array (TP(0..n) then FP(0..n)), None without validation triples."""
    ptr = L.get_TPFP(r, vpos.ctypes.data, vneg.ctypes.data, tpos.ctypes.data, tneg.ctypes.data)
    if not ptr:
        return None
    n = L.get_n_interval(r, vpos.ctypes.data, vneg.ctypes.data)
    return np.ctypeslib.as_array(ptr, shape=(2 * (n + 1),)).copy()


def reference_roc_lists(res, n_intervals, total):
    """Config.py:536-556 of the reference, restated literally: `res` = get_TPFP's list, `total` = the length of the test list."""
    TPR = []
    FPR = []
    if res[0] != 0 or res[0 + n_intervals + 1] != 0:
        TPR.append(0)
        FPR.append(0)
    for i in range(0, n_intervals + 1):
        TPR.append(res[i])
        FPR.append(res[i + n_intervals + 1])
    if TPR[len(TPR) - 1] != total or FPR[len(FPR) - 1] != total:
        TPR.append(total)
        FPR.append(total)
    for i in range(len(TPR)): TPR[i] /= TPR[-1]
    for i in range(len(FPR)): FPR[i] /= FPR[-1]
    trapz = getattr(np, "trapezoid", None) or np.trapz
    return TPR, FPR, trapz(TPR, FPR)
