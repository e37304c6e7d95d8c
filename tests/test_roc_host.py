"""ROC counts and AUC, the part that needs no GPU: the algorithm kge_tc_roc implements (csrc/tclass.hip) restated
in NumPy equals the library's host get_TPFP element for element, its integer area equals the trapezoid sum over the explicit
point list, and Config._roc_lists builds the reference's plot_roc lists."""
import os

import numpy as np
import pytest

import roc_cases as rc
import tclass_cases as tc
from conftest import GOLDEN
from openkeonspark_amd import _lib
from openkeonspark_amd.Config import Config

MIN_COMPARED = {"kg_tiny": 4, "kg_small": 12}


def open_fixture(kg):
    z = np.load(os.path.join(GOLDEN, "tc_%s.npz" % kg))
    L = _lib.lib()
    L.kge_set_option(b"libc_rand_restart", 1)
    con = Config()
    con.set_in_path(os.path.join(GOLDEN, kg))
    con.set_work_threads(1)
    con.set_test_link_prediction(True)
    con.init()
    rc.declare(L)
    scores = tuple(np.ascontiguousarray(z[k]) for k in ("vpos", "vneg", "tpos", "tneg"))
    return z, L, con, scores


def check_against_host(L, R, valid_rel, test_rel, scores):
    vpos, vneg, tpos, tneg = scores
    got = rc.numpy_roc(valid_rel, vpos, vneg, test_rel, tpos, tneg)
    for r in range(R):
        want = rc.host_tpfp(L, r, vpos, vneg, tpos, tneg)
        if want is None:
            assert r not in got
            continue
        tp, fp, area2, n_r, n = got[r]
        assert n == L.get_n_interval(r, vpos.ctypes.data, vneg.ctypes.data)
        assert np.array_equal(np.concatenate([tp, fp]), want), r
        assert area2 == (rc.trapezoid2(tp, fp, n_r) if n_r else 0), r
        assert n_r == int((test_rel == r).sum())
    return got


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_equals_host_get_tpfp_on_the_adversarial_lists(tmp_path, seed):
    path = rc.write_lists_dir(str(tmp_path / "lists"))
    L, con, V, T, R = tc.open_lists(path)
    rc.declare(L)
    assert T == rc.TEST_TOTAL
    valid_rel, test_rel = rc.sorted_relations()
    got = check_against_host(L, R, valid_rel, test_rel, rc.adversarial_scores(seed))
    # the cases are what they claim to be
    assert got[3][4] == 0 and got[7][4] + 2 > tc.LDS_BINS and got[4][4] + 2 <= tc.LDS_BINS and got[10][4] + 2 <= tc.LDS_BINS
    assert got[5][3] == 0 and not got[5][0].any() and 6 not in got
    assert rc.SHAPES[4][1] == tc.FUSED_MAX_TRIPLES and rc.SHAPES[7][1] == tc.FUSED_MAX_TRIPLES + 1
    for r in (0, 4, 7, 10):      # scores below the grid's origin and above its last point: neither end of the curve is trivial
        tp, fp, _, n_r, _ = got[r]
        assert 0 < tp[0] and tp[-1] < n_r and 0 < fp[0] and fp[-1] < n_r, r


@pytest.mark.parametrize("kg", ["kg_tiny", "kg_small"])
def test_restatement_equals_host_get_tpfp_and_the_reference_fixture(kg):
    z, L, con, scores = open_fixture(kg)
    valid_rel, test_rel = z["valid"][2], z["test"][2]
    got = check_against_host(L, con.relTotal, valid_rel, test_rel, scores)
    compared = 0
    for r, (tp, fp, _, n_r, _) in got.items():
        if n_r == 0:      # the fixture records the reference's out-of-bounds reads there
            continue
        assert np.array_equal(np.concatenate([tp, fp]), z["tpfp_%d" % r]), r
        compared += 1
    assert compared >= MIN_COMPARED[kg]


@pytest.mark.parametrize("kg", ["kg_tiny", "kg_small"])
def test_roc_lists_are_the_reference_plot_roc_lists(kg):
    z = np.load(os.path.join(GOLDEN, "tc_%s.npz" % kg))
    total = z["test"].shape[1]
    test_rels = set(z["test"][2].tolist())
    compared = 0
    for key in z.files:
        if not key.startswith("tpfp_") or int(key[5:]) not in test_rels:
            continue
        counts = z[key]
        n = len(counts) // 2 - 1
        want = rc.reference_roc_lists([int(c) for c in counts], n, total)
        got = Config._roc_lists(counts, n, total)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], key
        assert isinstance(got[0], list) and got[0][-1] == 1.0 and got[1][-1] == 1.0
        compared += 1
    assert compared >= MIN_COMPARED[kg]
    # a one-relation list whose last grid point counts everything and whose first counts something: only the start point is added
    assert Config._roc_lists([1, 2, 1, 2], 1, 2) == ([0.0, 0.5, 1.0], [0.0, 0.5, 1.0], 0.5)
    assert Config._roc_lists([0, 2, 0, 1], 1, 2)[0] == [0.0, 1.0, 1.0]      # no start point, an end point

