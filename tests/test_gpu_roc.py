"""ROC counts and AUC on the device (kge_tc_roc, Config.roc_auc / roc_curve / plot_roc) against the compiled reference's recorded
get_TPFP outputs (tests/golden/tc_*.npz) and the library's host get_TPFP: integer counts and one division of integers, so every
comparison is exact."""
import os

import numpy as np
import pytest

import roc_cases as rc
import tclass_cases as tc
from conftest import GOLDEN
from openkeonspark_amd import _lib
from openkeonspark_amd.Config import Config, KgeError

pytestmark = pytest.mark.gpu

KGE_ERR_NO_DATASET, KGE_ERR_BAD_ARG, KGE_ERR_UNSUPPORTED = -2, -3, -4
FILL, MARGIN = -9, 64


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_roc(L, R, split, vpos, vneg, pos, neg, capacity=None, n_valid=None, n=None):
    """kge_tc_roc on uploaded scores with every output pre-filled -> (rc, auc2 [R, 2], tpfp with MARGIN spare elements or
    None, h_offsets).  capacity None = d_tpfp NULL; "fit" = a first NULL call sizes the buffer."""
    import torch
    dvp, dvn = dev(vpos), dev(vneg)
    dp, dn = (dvp, dvn) if pos is vpos else (dev(pos), dev(neg))
    n_valid = len(vpos) if n_valid is None else n_valid
    n = len(pos) if n is None else n
    offsets = np.full(R + 1, FILL, np.int64)
    if capacity == "fit":
        auc2 = torch.full((R, 2), FILL, dtype=torch.int64, device="cuda")
        rc_ = L.kge_tc_roc(dvp.data_ptr(), dvn.data_ptr(), n_valid, split, dp.data_ptr(), dn.data_ptr(), n, auc2.data_ptr(), None, 0,
                           offsets.ctypes.data, None)
        assert rc_ == 0, _lib.last_error(L)
        capacity = int(offsets[R])
    auc2 = torch.full((R, 2), FILL, dtype=torch.int64, device="cuda")
    tpfp = None if capacity is None else torch.full((capacity + MARGIN,), FILL, dtype=torch.int64, device="cuda")
    rc_ = L.kge_tc_roc(dvp.data_ptr(), dvn.data_ptr(), n_valid, split, dp.data_ptr(), dn.data_ptr(), n, auc2.data_ptr(),
                       None if tpfp is None else tpfp.data_ptr(), 0 if capacity is None else capacity, offsets.ctypes.data, None)
    torch.cuda.synchronize()
    return rc_, auc2.cpu().numpy(), None if tpfp is None else tpfp.cpu().numpy(), offsets


def check_outputs(R, want, auc2, tpfp, offsets):
    """want = numpy_roc's dict.  Every slice, both numbers of every relation, the offsets and the margin beyond them."""
    at = 0
    for r in range(R):
        assert offsets[r] == at, r
        if r in want:
            tp, fp, area2, n_r, n = want[r]
            assert np.array_equal(tpfp[at:at + 2 * (n + 1)], np.concatenate([tp, fp])), r
            assert (int(auc2[r, 0]), int(auc2[r, 1])) == ((area2, n_r) if n_r else (0, 0)), r
            at += 2 * (n + 1)
        else:
            assert tuple(auc2[r]) == (0, 0), r
    assert offsets[R] == at and (tpfp[at:] == FILL).all() and len(tpfp) == at + MARGIN


@pytest.mark.parametrize("kg", ["kg_tiny", "kg_small"])
def test_counts_match_the_reference_fixture(kg):
    z = np.load(os.path.join(GOLDEN, "tc_%s.npz" % kg))
    L = _lib.lib()
    L.kge_set_option(b"libc_rand_restart", 1)
    con = Config()
    con.set_in_path(os.path.join(GOLDEN, kg))
    con.set_work_threads(1)
    con.set_test_link_prediction(True)
    con.init()
    R = con.relTotal
    vpos, vneg, tpos, tneg = (np.ascontiguousarray(z[k]) for k in ("vpos", "vneg", "tpos", "tneg"))
    rc_, auc2, tpfp, offsets = device_roc(L, R, 1, vpos, vneg, tpos, tneg, capacity="fit")
    assert rc_ == 0, _lib.last_error(L)
    valid_rel, test_rel = z["valid"][2], z["test"][2]
    has_valid = np.isin(np.arange(R), valid_rel)
    assert np.array_equal(np.diff(offsets), np.where(has_valid, 2 * (z["n_interval"] + 1), 0))
    compared = 0
    for r in set(test_rel.tolist()) & set(valid_rel.tolist()):      # without test triples the fixture holds out-of-bounds reads
        assert np.array_equal(tpfp[offsets[r]:offsets[r + 1]], z["tpfp_%d" % r]), r
        compared += 1
    assert compared >= {"kg_tiny": 4, "kg_small": 12}[kg]
    check_outputs(R, rc.numpy_roc(valid_rel, vpos, vneg, test_rel, tpos, tneg), auc2, tpfp, offsets)


@pytest.fixture(scope="module")
def lists_dir(tmp_path_factory):
    return rc.write_lists_dir(str(tmp_path_factory.mktemp("roc") / "lists"))


@pytest.mark.parametrize("seed", [0, 1])
def test_adversarial_lists_match_the_host_routine(lists_dir, seed):
    L, con, V, T, R = tc.open_lists(lists_dir)
    rc.declare(L)
    valid_rel, test_rel = rc.sorted_relations()
    vpos, vneg, tpos, tneg = rc.adversarial_scores(seed)
    n_host = np.array([L.get_n_interval(r, vpos.ctypes.data, vneg.ctypes.data) for r in range(R)])
    assert n_host[7] + 2 > tc.LDS_BINS and n_host[4] + 2 <= tc.LDS_BINS and L.getTestTotal() == 64507      # the paths meant
    assert n_host[3] == 0 and n_host[10] + 2 <= tc.LDS_BINS and rc.SHAPES[10][1] > tc.FUSED_MAX_TRIPLES
    for split, rel_of, pos, neg in ((1, test_rel, tpos, tneg), (0, valid_rel, vpos, vneg)):
        want = rc.numpy_roc(valid_rel, vpos, vneg, rel_of, pos, neg)
        rc_, auc2, tpfp, offsets = device_roc(L, R, split, vpos, vneg, pos, neg, capacity="fit")
        assert rc_ == 0, _lib.last_error(L)
        if split == 1:
            for r in range(R):
                host = rc.host_tpfp(L, r, vpos, vneg, tpos, tneg)
                if host is None:
                    assert offsets[r] == offsets[r + 1] and r not in want
                else:
                    bad = int((tpfp[offsets[r]:offsets[r + 1]] != host).sum())
                    print("relation", r, "n_interval", n_host[r], "elements differing from get_TPFP:", bad)
                    assert bad == 0 and len(host) == offsets[r + 1] - offsets[r]
            assert tuple(auc2[5]) == (0, 0) and not tpfp[offsets[5]:offsets[6]].any() and offsets[6] == offsets[7]
        check_outputs(R, want, auc2, tpfp, offsets)
        rc_, auc_only, none, offsets_only = device_roc(L, R, split, vpos, vneg, pos, neg)
        assert rc_ == 0 and none is None and np.array_equal(auc_only, auc2) and np.array_equal(offsets_only, offsets)


def make_config(model, dim=32):
    """test_gpu_tclass.py's recipe: kg_small, every Config from the libc rand() state of a fresh process."""
    import openkeonspark_amd as pkg
    L = _lib.lib()
    rc.declare(L)
    L.kge_set_option(b"libc_rand_restart", 1)
    con = Config()
    con.set_in_path(os.path.join(GOLDEN, "kg_small"))
    con.set_work_threads(1)
    con.set_dimension(dim)
    con.set_test_triple_classification(True)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    return con


def widen(con, seed):
    """Random tables with score ranges of a trained model's order (the initial ones give grids of a few points)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    for t in con._tables:
        t.copy_((torch.rand(t.shape, generator=g) * 2 - 1).to(t.device) * 0.6)
    con.tables_changed()


def host_scores(con):
    """test_step's scores of the batches the Config's last draw left in its buffers."""
    f = lambda h, t, r: np.ascontiguousarray(con.test_step(h, t, r).reshape(-1), dtype=np.float32)
    return (f(con.valid_pos_h, con.valid_pos_t, con.valid_pos_r), f(con.valid_neg_h, con.valid_neg_t, con.valid_neg_r),
            f(con.test_pos_h, con.test_pos_t, con.test_pos_r), f(con.test_neg_h, con.test_neg_t, con.test_neg_r))


@pytest.mark.parametrize("model", ["TransE", "TransH", "TransD", "TransR"])
def test_config_methods_equal_the_host_routine(model, tmp_path):
    import torch
    L = _lib.lib()
    con = make_config(model)
    widen(con, 11)
    before = [t.clone() for t in con._tables]
    res = con.roc_auc()
    ref = make_config(model)
    widen(ref, 11)
    ref.triple_classification()
    assert np.array_equal(con.test_neg_t, ref.test_neg_t) and np.array_equal(con.valid_neg_t, ref.valid_neg_t)
    assert np.array_equal(con.test_neg_h, ref.test_neg_h) and np.array_equal(con.valid_neg_h, ref.valid_neg_h)
    vpos, vneg, tpos, tneg = host_scores(con)
    R = con.relTotal
    want = rc.numpy_roc(con.valid_pos_r, vpos, vneg, con.test_pos_r, tpos, tneg)
    for r in range(R):
        n_r = want[r][3] if r in want else 0
        assert res["n"][r] == n_r
        if n_r:
            assert res["auc"][r] == want[r][2] / (2 * n_r * n_r), r
        else:
            assert np.isnan(res["auc"][r])
    have = res["n"] > 0
    assert have.sum() >= 12 and res["auc"].dtype == np.float64 and res["n"].dtype == np.int64
    assert res["macro"] == float(res["auc"][have].mean())
    assert res["weighted"] == float((res["n"][have] * res["auc"][have]).sum() / res["n"][have].sum())
    print(model, "macro", res["macro"], "weighted", res["weighted"], "grid sizes up to", max(w[4] for w in want.values()))
    # curves: every relation with validation triples, against the host routine on test_step's scores of the batches then drawn
    curves = 0
    for r in range(R):
        if r not in want:
            with pytest.raises(KgeError):
                con.roc_curve(r)
            continue
        c = con.roc_curve(r)
        vpos, vneg, tpos, tneg = host_scores(con)
        host = rc.host_tpfp(L, r, vpos, vneg, tpos, tneg)
        n = len(host) // 2 - 1
        assert np.array_equal(c["tp"], host[:n + 1]) and np.array_equal(c["fp"], host[n + 1:]), r
        mn = min(vpos[con.valid_pos_r == r].min(), vneg[con.valid_pos_r == r].min())
        assert c["thresholds"].dtype == np.float32 and c["thresholds"].tobytes() == tc.fma32(np.arange(n + 1), mn).tobytes()
        n_r = int((con.test_pos_r == r).sum())
        assert c["n"] == n_r
        if n_r:
            assert np.array_equal(c["tpr"], host[:n + 1] / n_r) and np.array_equal(c["fpr"], host[n + 1:] / n_r)
            w = rc.numpy_roc(con.valid_pos_r, vpos, vneg, con.test_pos_r, tpos, tneg)[r]
            assert c["auc"] == w[2] / (2 * n_r * n_r)
        else:
            assert np.isnan(c["auc"])
        curves += 1
    assert curves >= 12
    first = min(want)
    cv = con.roc_curve(first, split="valid")
    vpos, vneg, _, _ = host_scores(con)
    w = rc.numpy_roc(con.valid_pos_r, vpos, vneg, con.valid_pos_r, vpos, vneg)[first]      # the validation scores on their own grid
    assert np.array_equal(cv["tp"], w[0]) and np.array_equal(cv["fp"], w[1]) and cv["n"] == w[3] == int((con.valid_pos_r == first).sum())
    assert cv["auc"] == w[2] / (2 * w[3] * w[3]) and len(cv["tp"]) == len(cv["thresholds"])
    with pytest.raises(KgeError):
        con.roc_auc("train")
    for t, b in zip(con._tables, before):
        assert torch.equal(t, b)


@pytest.mark.parametrize("model", ["TransE", "TransH", "TransD", "TransR"])
def test_plot_roc_is_the_reference_construction(model, tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    L = _lib.lib()
    con = make_config(model)
    widen(con, 11)
    z = np.load(os.path.join(GOLDEN, "tc_kg_small.npz"))
    both = sorted(set(z["valid"][2].tolist()) & set(z["test"][2].tolist()))
    for k, r in enumerate((both[0], both[-1])):
        fig = str(tmp_path / ("roc%d.png" % k))
        FPR, TPR, auc = con.plot_roc(int(r), fig)
        plt.close("all")
        vpos, vneg, tpos, tneg = host_scores(con)
        host = rc.host_tpfp(L, int(r), vpos, vneg, tpos, tneg)
        want = rc.reference_roc_lists([int(c) for c in host], len(host) // 2 - 1, len(tpos))
        assert TPR == want[0] and FPR == want[1] and auc == want[2], r
        assert os.path.getsize(fig) > 0


def test_a_refused_relation_index_draws_nothing():
    con = make_config("TransE")      # every make_config restarts the libc rand() sequence
    for bad in (-1, con.relTotal):
        with pytest.raises(KgeError):
            con.roc_curve(bad)
    con.roc_auc()
    ref = make_config("TransE")
    ref.roc_auc()
    for name in ("test_neg_h", "test_neg_t", "valid_neg_h", "valid_neg_t"):
        assert np.array_equal(getattr(con, name), getattr(ref, name)), name


def test_driver_adds_the_two_roc_metrics(tmp_path):
    import json
    import openkeonspark_amd.distribute_training as dt
    kg = os.path.join(GOLDEN, "kg_small")
    results = {}

    def refuse(name):
        raise ValueError("%s in lp_results.json is not JSON" % name)
    for flag in ("0", "1"):
        out = str(tmp_path / ("drv" + flag))
        os.makedirs(out)
        args = dt.parse_args(["--input_path", kg, "--output_path", out, "--embedding_dimension", "16", "--mode", "test", "--test_roc", flag])
        returned = dt.main_fun(args)
        results[flag] = json.load(open(os.path.join(out, "lp_results.json")), parse_constant=refuse)
        assert set(returned) == set(results[flag])
    assert set(results["1"]) == set(results["0"]) | {"roc_auc_macro", "roc_auc_weighted"}
    assert not any(k.startswith("roc") for k in results["0"])
    assert 0.0 <= results["1"]["roc_auc_macro"] <= 1.0 and 0.0 <= results["1"]["roc_auc_weighted"] <= 1.0
    assert dt.parse_args(["--input_path", kg]).test_roc == 0


def test_errors_leave_everything_untouched(lists_dir, tmp_path):
    L, con, V, T, R = tc.open_lists(lists_dir)
    rc.declare(L)
    vpos, vneg, tpos, tneg = rc.adversarial_scores(4)
    inside_r4 = 300 + 1 + 2 + 5 + 17          # a validation position inside relation 4
    test_r0 = 123                              # a test position inside relation 0

    def untouched(out, offsets_filled=False):
        rc_, auc2, tpfp, offsets = out
        assert (auc2 == FILL).all() and (tpfp is None or (tpfp == FILL).all())
        assert offsets_filled or (offsets == FILL).all()
        return rc_

    for poison in (np.nan, np.inf, -np.inf):
        bad = vneg.copy()
        bad[inside_r4] = poison
        assert untouched(device_roc(L, R, 1, vpos, bad, tpos, tneg, capacity=200000)) == KGE_ERR_BAD_ARG
        assert "non-finite validation score" in _lib.last_error(L)
        bad = tpos.copy()
        bad[test_r0] = poison
        assert untouched(device_roc(L, R, 1, vpos, vneg, bad, tneg, capacity=200000)) == KGE_ERR_BAD_ARG
        assert "non-finite" in _lib.last_error(L)
    wide = vneg.copy()
    wide[inside_r4] = 2.0e5                    # relation 4: (2e5 + 12) / 0.01 >= 2^24 grid points
    assert untouched(device_roc(L, R, 1, vpos, wide, tpos, tneg, capacity=200000)) == KGE_ERR_UNSUPPORTED
    assert "2^24" in _lib.last_error(L)
    assert untouched(device_roc(L, R, 1, vpos[:-1], vneg[:-1], tpos, tneg, capacity=200000)) == KGE_ERR_BAD_ARG
    assert untouched(device_roc(L, R, 1, vpos, vneg, tpos[:-1], tneg[:-1], capacity=200000)) == KGE_ERR_BAD_ARG
    assert untouched(device_roc(L, R, 0, vpos, vneg, tpos, tneg, capacity=200000)) == KGE_ERR_BAD_ARG      # the test list as split 0
    assert untouched(device_roc(L, R, 2, vpos, vneg, tpos, tneg, capacity=200000)) == KGE_ERR_BAD_ARG
    ok = device_roc(L, R, 1, vpos, vneg, tpos, tneg)
    assert ok[0] == 0
    total = int(ok[3][R])
    short = device_roc(L, R, 1, vpos, vneg, tpos, tneg, capacity=total - 1)
    assert untouched(short, offsets_filled=True) == KGE_ERR_BAD_ARG and np.array_equal(short[3], ok[3])
    assert "tpfp_capacity" in _lib.last_error(L)
    offsets = np.zeros(R + 1, np.int64)
    assert L.kge_tc_roc(None, None, V, 1, None, None, T, None, None, 0, offsets.ctypes.data, None) == KGE_ERR_BAD_ARG
    # before importTestFiles (a failed import leaves the library without evaluation lists): the host routines' message
    empty = tmp_path / "train_only"
    os.makedirs(str(empty))
    L.setInPath((str(empty) + "/").encode())
    L.kge_clear_error()
    L.importTestFiles()
    L.kge_clear_error()
    assert untouched(device_roc(L, R, 1, vpos, vneg, tpos, tneg, capacity=200000)) == KGE_ERR_NO_DATASET
    assert _lib.last_error(L) == "triple classification: importTestFiles has not been called"
    L.kge_clear_error()


def test_a_fit_after_a_roc_call_gives_the_host_thresholds(lists_dir):
    import torch
    L, con, V, T, R = tc.open_lists(lists_dir)
    vpos, vneg, tpos, tneg = rc.adversarial_scores(0)
    assert device_roc(L, R, 1, vpos, vneg, tpos, tneg, capacity="fit")[0] == 0
    want = tc.host_fit(L, R, vpos, vneg)
    dp, dn = dev(vpos), dev(vneg)
    thresh = torch.full((R,), -1.0, dtype=torch.float32, device="cuda")
    assert L.kge_tc_fit(dp.data_ptr(), dn.data_ptr(), V, thresh.data_ptr(), None, None) == 0, _lib.last_error(L)
    torch.cuda.synchronize()
    assert thresh.cpu().numpy().tobytes() == want.tobytes()
    rc_, auc2, _, _ = device_roc(L, R, 1, vpos, vneg, tpos, tneg)      # and a ROC call after a fit
    valid_rel, test_rel = rc.sorted_relations()
    want_roc = rc.numpy_roc(valid_rel, vpos, vneg, test_rel, tpos, tneg)
    assert rc_ == 0 and all(int(auc2[r, 0]) == w[2] for r, w in want_roc.items())
