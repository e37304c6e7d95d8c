"""Device triple classification, the part that needs no GPU: the entry points refuse to run without a device and write
nothing, and the algorithm csrc/tclass.hip implements -- bin every score once at k(s) = min{ i : s <= g(i) }, prefix sum,
arg-max under the host's float tie rule -- restated in NumPy equals the host's grid search (getBestThreshold) byte for byte
on score sets aimed at the grid's boundaries."""
import ctypes

import numpy as np
import pytest

import tclass_cases as tc
from openkeonspark_amd import _lib

KGE_ERR_NO_DEVICE = -1


def test_fma32_is_single_rounded():
    """The restatement's grid point against exact rational arithmetic rounded once to float32."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    step = Fraction(float(tc.INTERVAL))
    for mn in (np.float32(0.25), np.float32(-150.0), np.float32(-3.0000002), np.float32(1e-3), np.float32(19.37)):
        i = np.concatenate([np.arange(0, 300), rng.integers(0, 1 << 24, 3000)])
        got = tc.fma32(i, mn)
        for ii, g in zip(i.tolist(), got.tolist()):
            exact = Fraction(ii) * step + Fraction(float(mn))
            lo, hi = np.nextafter(np.float32(g), np.float32(-np.inf)), np.nextafter(np.float32(g), np.float32(np.inf))
            err = abs(Fraction(g) - exact)
            # nearest: no neighbour is closer (a tie goes to the even mantissa, which the neighbours' errors cannot beat)
            assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (ii, float(mn))
        assert (np.diff(tc.fma32(np.arange(0, 70000), mn)) >= 0).all()      # the monotonicity the binning rests on


def test_entry_points_without_a_device(tmp_path):
    L = _lib.lib()
    if L.kge_device_available():
        pytest.skip("a device is present: tests/test_gpu_tclass.py covers the entry points")
    path = tc.write_lists_dir(str(tmp_path / "lists"), shapes=[(3, 2), (2, 2)])
    L, con, V, T, R = tc.open_lists(path)
    pos, neg = np.arange(V, dtype=np.float32), np.arange(V, dtype=np.float32) + 1
    thresh = np.full(R, -7.0, np.float32)
    nint = np.full(R, -7, np.int32)
    counts = np.full(4, -7, np.int64)
    rel = np.full((R, 2), -7, np.int64)
    assert L.kge_tc_fit(pos.ctypes.data, neg.ctypes.data, V, thresh.ctypes.data, nint.ctypes.data, None) == KGE_ERR_NO_DEVICE
    tpos, tneg = np.zeros(T, np.float32), np.ones(T, np.float32)
    assert L.kge_tc_apply(1, thresh.ctypes.data, tpos.ctypes.data, tneg.ctypes.data, T, counts.ctypes.data, rel.ctypes.data,
                          None) == KGE_ERR_NO_DEVICE
    L.kge_clear_error()
    assert (thresh == -7).all() and (nint == -7).all() and (counts == -7).all() and (rel == -7).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_binning_rule_equals_the_host_grid_search(tmp_path, seed):
    path = tc.write_lists_dir(str(tmp_path / "lists"))
    L, con, V, T, R = tc.open_lists(path)
    valid_rel, test_rel = tc.sorted_relations()
    assert V == len(valid_rel) and T == len(test_rel)
    vpos, vneg, tpos, tneg = tc.adversarial_scores(seed=seed)
    want = tc.host_fit(L, R, vpos, vneg)
    got = np.full(R, -1.0, np.float32)
    n_interval = tc.numpy_fit(valid_rel, vpos, vneg, got)
    assert got.tobytes() == want.tobytes(), np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    for r in range(R):
        assert L.get_n_interval(r, vpos.ctypes.data, vneg.ctypes.data) == n_interval.get(r, 0)
    # the cases are what they claim to be
    assert n_interval[7] == 0                                     # min == max
    assert n_interval[8] + 2 > tc.LDS_BINS                        # wider than the LDS histogram
    assert n_interval[4] + 2 <= tc.LDS_BINS and tc.SHAPES[4][0] <= tc.FUSED_MAX_TRIPLES
    assert tc.SHAPES[0][0] >= 50000 and tc.SHAPES[10][0] > tc.FUSED_MAX_TRIPLES
    assert want[6] == -1.0 and 5 not in test_rel                  # no validation triples: untouched; r5 has no test triples
    assert (vpos < 0).any() and (want < 0).any()
    # the host's accuracy from the thresholds against the counts the device's rule gives
    acc = np.zeros(1, np.float32)
    L.test_triple_classification(want.ctypes.data, tpos.ctypes.data, tneg.ctypes.data, acc.ctypes.data)
    tp, tn, fp, fn = tc.host_counts(want, valid_rel, test_rel, tpos, tneg)
    assert np.float32(1.0 * (tp + tn) / (tp + tn + fp + fn)).tobytes() == acc.tobytes()
