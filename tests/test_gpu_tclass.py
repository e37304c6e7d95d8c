"""Triple classification on the device (kge_tc_fit / kge_tc_apply, Config.triple_classification / validation_accuracy) against
the compiled reference's recorded outputs (tests/golden/tc_*.npz) and against the library's host routines, bit for bit."""
import os

import numpy as np
import pytest

import tclass_cases as tc
from conftest import GOLDEN
from openkeonspark_amd import _lib
from openkeonspark_amd.Config import Config

pytestmark = pytest.mark.gpu

KGE_ERR_NO_DATASET, KGE_ERR_BAD_ARG, KGE_ERR_UNSUPPORTED = -2, -3, -4


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_fit(L, R, vpos, vneg, fill=-1.0):
    """kge_tc_fit on uploaded scores -> (rc, thresholds, n_interval) with both outputs pre-filled."""
    import torch
    dp, dn = dev(vpos), dev(vneg)
    thresh = torch.full((R,), fill, dtype=torch.float32, device="cuda")
    nint = torch.full((R,), -9, dtype=torch.int32, device="cuda")
    rc = L.kge_tc_fit(dp.data_ptr(), dn.data_ptr(), len(vpos), thresh.data_ptr(), nint.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, thresh, nint


def device_apply(L, R, split, thresh, pos, neg):
    import torch
    dp, dn = dev(pos), dev(neg)
    counts = torch.full((4,), -9, dtype=torch.int64, device="cuda")
    rel = torch.full((R, 2), -9, dtype=torch.int64, device="cuda")
    rc = L.kge_tc_apply(split, thresh.data_ptr(), dp.data_ptr(), dn.data_ptr(), len(pos), counts.data_ptr(), rel.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy(), rel.cpu().numpy()


def acc32(counts):
    tp, tn, fp, fn = (int(x) for x in counts)
    return np.float32(1.0 * (tp + tn) / (tp + tn + fp + fn))


@pytest.mark.parametrize("kg", ["kg_tiny", "kg_small"])
def test_stages_match_the_reference_fixture(kg):
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
    rc, thresh, nint = device_fit(L, R, vpos, vneg)
    assert rc == 0, _lib.last_error(L)
    got = thresh.cpu().numpy()
    print("thresholds differing from the fixture:", int((got.view(np.int32) != z["thresh"].view(np.int32)).sum()), "of", R)
    assert got.tobytes() == z["thresh"].astype(np.float32).tobytes()      # untouched (-1) where the fixture's are
    assert np.array_equal(nint.cpu().numpy(), z["n_interval"])
    rc, counts, rel = device_apply(L, R, 1, thresh, tpos, tneg)
    assert rc == 0, _lib.last_error(L)
    print("device accuracy", acc32(counts), "fixture", z["acc"])
    assert acc32(counts).tobytes() == z["acc"].astype(np.float32).tobytes()
    assert rel[:, 0].sum() == counts[0] + counts[1] and rel[:, 1].sum() == counts.sum()


@pytest.mark.parametrize("seed", [0, 1])
def test_adversarial_scores_match_the_host_routines(tmp_path, seed):
    path = tc.write_lists_dir(str(tmp_path / "lists"))
    L, con, V, T, R = tc.open_lists(path)
    valid_rel, test_rel = tc.sorted_relations()
    vpos, vneg, tpos, tneg = tc.adversarial_scores(seed=seed)
    want = tc.host_fit(L, R, vpos, vneg)
    rc, thresh, nint = device_fit(L, R, vpos, vneg)
    assert rc == 0, _lib.last_error(L)
    got = thresh.cpu().numpy()
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    print("relations whose threshold differs from getBestThreshold:", bad.tolist())
    assert got.tobytes() == want.tobytes()
    n_host = np.array([L.get_n_interval(r, vpos.ctypes.data, vneg.ctypes.data) for r in range(R)])
    assert np.array_equal(nint.cpu().numpy(), n_host)
    assert n_host[7] == 0 and n_host[8] + 2 > tc.LDS_BINS and n_host[4] + 2 <= tc.LDS_BINS      # min == max; global and LDS histograms
    for split, rel_of, pos, neg in ((1, test_rel, tpos, tneg), (0, valid_rel, vpos, vneg)):
        rc, counts, rel = device_apply(L, R, split, thresh, pos, neg)
        assert rc == 0, _lib.last_error(L)
        assert tuple(counts.tolist()) == tc.host_counts(want, valid_rel, rel_of, pos, neg)
        keep = np.isin(rel_of, np.unique(valid_rel))
        th = want[rel_of]
        right = np.bincount(rel_of[keep], ((pos <= th).astype(np.int64) + (neg > th))[keep], R).astype(np.int64)
        assert np.array_equal(rel[:, 0], right) and np.array_equal(rel[:, 1], 2 * np.bincount(rel_of[keep], minlength=R))
        if split == 1:
            acc = np.zeros(1, np.float32)
            L.test_triple_classification(want.ctypes.data, pos.ctypes.data, neg.ctypes.data, acc.ctypes.data)
            assert acc32(counts).tobytes() == acc.tobytes()
    assert rel[6, 1] == 0 and tc.SHAPES[6] == (0, 50)          # test triples of a relation without validation triples are not counted


def make_config(model, dim=32):
    import openkeonspark_amd as pkg
    L = _lib.lib()
    tc.declare(L)
    L.kge_set_option(b"libc_rand_restart", 1)      # every Config of a test starts from the libc rand() state of a fresh process
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


@pytest.mark.parametrize("model", ["TransE", "TransH", "TransD", "TransR"])
def test_config_paths_equal_the_host_paths(model):
    import torch
    L = _lib.lib()
    con = make_config(model)
    widen(con, 11)
    before = [t.clone() for t in con._tables]
    acc = con.validation_accuracy()
    valid = con._tc_valid_drawn
    # the early-stop check's formula as it stood before the device path (distribute_training._validation_accuracy)
    ph, pt, pr, nh, nt, nr = valid
    pos = np.ascontiguousarray(con.test_step(ph, pt, pr).reshape(-1), dtype=np.float32)
    neg = np.ascontiguousarray(con.test_step(nh, nt, nr).reshape(-1), dtype=np.float32)
    thresh = np.zeros(con.relTotal, np.float32)
    L.getBestThreshold(thresh.ctypes.data, pos.ctypes.data, neg.ctypes.data)
    want = float((pos <= thresh[pr]).sum() + (neg > thresh[nr]).sum()) / (2.0 * max(len(pos), 1))
    print(model, "validation accuracy", acc, "host formula", want, "grid sizes up to",
          max(L.get_n_interval(r, pos.ctypes.data, neg.ctypes.data) for r in range(con.relTotal)))
    assert acc == want
    import openkeonspark_amd.distribute_training as dt
    arrays = [np.array(a) for a in valid]
    assert dt._validation_accuracy(con, arrays) == want and con._tc_valid_dev[0] is arrays
    ids = con._tc_valid_dev[1]
    assert con.validation_accuracy(arrays) == want and con._tc_valid_dev[1] is ids          # ids stay on the device
    rv = con.triple_classification("valid")                      # draws new negatives (left in con.valid_neg_*) and refits
    pos = np.ascontiguousarray(con.test_step(con.valid_pos_h, con.valid_pos_t, con.valid_pos_r).reshape(-1), dtype=np.float32)
    neg = np.ascontiguousarray(con.test_step(con.valid_neg_h, con.valid_neg_t, con.valid_neg_r).reshape(-1), dtype=np.float32)
    L.getBestThreshold(thresh.ctypes.data, pos.ctypes.data, neg.ctypes.data)
    assert rv["tp"] == (pos <= thresh[con.valid_pos_r]).sum() and rv["tn"] == (neg > thresh[con.valid_neg_r]).sum()
    assert rv["tp"] + rv["fn"] == len(pos) == rv["tn"] + rv["fp"] and con.relThresh.tobytes() == thresh.tobytes()
    assert con.validation_accuracy(arrays) == want               # the cached batch is not the redrawn one

    dev_con = make_config(model)
    widen(dev_con, 11)
    res = dev_con.triple_classification()
    host_con = make_config(model)
    widen(host_con, 11)
    host = host_con.test()
    print(model, "device", res, "host", host)
    assert res["acc"] == host["acc"]
    assert dev_con.relThresh.tobytes() == host_con.relThresh.tobytes()
    assert np.array_equal(dev_con.test_neg_t, host_con.test_neg_t) and np.array_equal(dev_con.valid_neg_t, host_con.valid_neg_t)
    assert res["tp"] + res["fn"] == res["tn"] + res["fp"] and res["precision"] == res["tp"] / (res["tp"] + res["fp"])
    for t, b in zip(con._tables, before):
        assert torch.equal(t, b)


def test_errors_leave_everything_untouched(tmp_path):
    import torch
    con = make_config("TransE")
    before = [t.clone() for t in con._tables]
    L = _lib.lib()
    path = tc.write_lists_dir(str(tmp_path / "lists"))
    L, lists_con, V, T, R = tc.open_lists(path)
    vpos, vneg, tpos, tneg = tc.adversarial_scores(seed=4)
    for poison in (np.nan, np.inf, -np.inf):
        bad = vneg.copy()
        bad[50000 + 1 + 2 + 3 + 17] = poison                      # inside relation 4; every other relation is in order
        rc, thresh, nint = device_fit(L, R, vpos, bad, fill=-5.0)
        assert rc == KGE_ERR_BAD_ARG and "non-finite" in _lib.last_error(L)
        assert (thresh.cpu().numpy() == -5.0).all()                # NO threshold written, not only the poisoned relation's
        assert (nint.cpu().numpy() == -9).all()
    wide = vneg.copy()
    wide[50000 + 1 + 2 + 3 + 17] = 2.0e5                          # relation 4: (2e5 + 12) / 0.01 >= 2^24 grid points
    rc, thresh, nint = device_fit(L, R, vpos, wide, fill=-5.0)
    assert rc == KGE_ERR_UNSUPPORTED and (thresh.cpu().numpy() == -5.0).all() and (nint.cpu().numpy() == -9).all()
    L.kge_clear_error()
    rc, thresh, nint = device_fit(L, R, vpos[:-1], vneg[:-1], fill=-5.0)
    assert rc == KGE_ERR_BAD_ARG and (thresh.cpu().numpy() == -5.0).all() and (nint.cpu().numpy() == -9).all()
    rc, thresh, _ = device_fit(L, R, vpos, vneg)
    assert rc == 0
    rc, counts, rel = device_apply(L, R, 1, thresh, tpos[:-1], tneg[:-1])
    assert rc == KGE_ERR_BAD_ARG and (counts == -9).all() and (rel == -9).all()
    rc, counts, rel = device_apply(L, R, 2, thresh, tpos, tneg)
    assert rc == KGE_ERR_BAD_ARG and (counts == -9).all()
    assert L.kge_tc_fit(None, None, V, thresh.data_ptr(), None, None) == KGE_ERR_BAD_ARG
    # before importTestFiles (a failed import leaves the library without evaluation lists): the host routines' message
    empty = tmp_path / "train_only"
    os.makedirs(str(empty))
    L.setInPath((str(empty) + "/").encode())
    L.kge_clear_error()
    L.importTestFiles()
    L.kge_clear_error()
    rc, thresh, _ = device_fit(L, R, vpos, vneg, fill=-5.0)
    assert rc == KGE_ERR_NO_DATASET and _lib.last_error(L) == "triple classification: importTestFiles has not been called"
    assert (thresh.cpu().numpy() == -5.0).all()
    rc, counts, _ = device_apply(L, R, 1, thresh, tpos, tneg)
    assert rc == KGE_ERR_NO_DATASET and (counts == -9).all()
    L.kge_clear_error()
    for t, b in zip(con._tables, before):
        assert torch.equal(t, b)
