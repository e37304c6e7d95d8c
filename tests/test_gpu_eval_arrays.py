"""Device build of the evaluation lists and of derived type lists (eval_build.hip) against the host build (kg_index.cpp
build_eval_lists / derive_type_lists, itself pinned to importTestFiles by tests/test_eval_arrays_host.py): every named array
identical, bit for bit, read back from the device copies the kernels read; then every evaluation entry point from an array
import against the same from the files."""
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from eval_arrays_cases import (array_config, assert_same_bits, n_n_lists, read_kg, read_type_file, snapshot, type_slices)
from openkeonspark_amd import _lib
from openkeonspark_amd.Config import Config

pytestmark = pytest.mark.gpu


def build(where, kg, train_on_device=False, **eval_kw):
    """where = "device" / "host" for the evaluation lists; train_on_device: the training index is built on the device too, so
    the evaluation build takes the training triples from the resident index instead of uploading them."""
    L = _lib.lib()
    _lib.check(L.kge_set_option(b"eval_index_device_min", 0 if where == "device" else -1), L)
    _lib.check(L.kge_set_option(b"index_device_min", 0 if train_on_device else -1), L)
    try:
        return array_config(kg, **eval_kw)
    finally:
        L.kge_set_option(b"eval_index_device_min", 1 << 22)
        L.kge_set_option(b"index_device_min", 1 << 22)


@pytest.mark.parametrize("kg_name", ["kg_tiny", "kg_small"])
def test_device_lists_equal_host_lists_on_golden_kgs(kg_name):
    kg = read_kg(kg_name)
    csr = read_type_file(os.path.join(kg["dir"], "type_constrain.txt"), kg["R"])
    for kw in (dict(type_lists=csr), dict(derive_types=True)):
        host = snapshot(build("host", kg, **kw).lib)
        dev = snapshot(build("device", kg, **kw).lib)
        assert len(host["head_type"]) > 0 and host["totals"][2] == len(host["all"])
        assert_same_bits(host, dev)
    assert type_slices(dev) == n_n_lists(kg["R"], kg["train"], kg["valid"], kg["test"])


def carve(E, R, n, seed, n_valid=None, n_test=None):
    """One draw of n triples cut into train / valid / test, a few training triples repeated in valid and in test."""
    from openkeonspark_amd.synthetic import generate_triples
    if R >= 100:      # a wide relation space: every tenth id stays without triples
        h, t, r = generate_triples(E, R - R // 10, n, seed, dup_frac=0.05)
        r = r + r // 9
    else:
        h, t, r = generate_triples(E, R, n, seed, dup_frac=0.05)
    nv = max(n // 10, 1) if n_valid is None else n_valid
    nt = max(n // 10, 1) if n_test is None else n_test
    n_tr = n - nv - nt
    rep = np.arange(0, n_tr, max(n_tr // 7, 1))[:7]
    cut = lambda lo, hi, extra: tuple(np.concatenate([a[lo:hi], a[rep]]) if extra else a[lo:hi].copy() for a in (h, t, r))
    return dict(E=E, R=R, train=cut(0, n_tr, False), valid=cut(n_tr, n_tr + nv, nv > 0), test=cut(n_tr + nv, n, nt > 0))


@pytest.mark.parametrize("E,R,n,seed,n_valid,n_test", [
    (50, 3, 4000, 1, None, None),            # heavy duplication
    (5000, 40, 60000, 2, None, None),
    (1, 1, 5, 4, None, None),
    (1024, 7, 3000, 6, None, None),          # bits(E) = 10 ...
    (1025, 7, 3000, 7, None, None),          # ... and 11: the packing boundary
    (200000, 1000, 300000, 5, None, None),   # wide ids, several sort blocks, relations without triples
    (50, 3, 4000, 8, 0, None),               # no validation triples
    (5000, 40, 6000, 9, None, 0),            # no test triples
])
def test_device_lists_equal_host_lists_random(E, R, n, seed, n_valid, n_test):
    kg = carve(E, R, n, seed, n_valid, n_test)
    host = snapshot(build("host", kg, derive_types=True).lib)
    dev = snapshot(build("device", kg, train_on_device=True, derive_types=True).lib)
    assert host["totals"].tolist() == [len(kg["test"][0]), len(kg["valid"][0]), sum(len(kg[s][0]) for s in ("train", "valid", "test"))]
    if n_valid == 0:
        assert len(host["valid"]) == 0
    if n_test == 0:
        assert len(host["test"]) == 0
    if R == 1000:      # relations without triples really were present, in the middle and at the end
        empty = host["head_lef"] == host["head_rig"]
        assert empty[9] and empty[R - 1] and not empty[0] and (empty == (host["tail_lef"] == host["tail_rig"])).all()
    a = host["all"]
    key = (a[:, 0].astype(np.int64) << 42) | (a[:, 1].astype(np.int64) << 21) | a[:, 2]
    assert (np.diff(key) >= 0).all() and (np.diff(key) == 0).any()      # sorted, duplicates kept
    assert_same_bits(host, dev)


def test_failed_device_import_leaves_the_old_state():
    kg = read_kg("kg_tiny")
    con = build("device", kg, derive_types=True)
    before = snapshot(con.lib)
    bad = [a.copy() for a in kg["test"]]
    bad[0][2] = kg["E"]
    L = con.lib
    L.kge_set_option(b"eval_index_device_min", 0)
    try:
        with pytest.raises(_lib.KgeError, match="test: id out of range at index 2"):
            con.init_evaluation_from_arrays(kg["valid"], bad)
    finally:
        L.kge_set_option(b"eval_index_device_min", 1 << 22)
    assert_same_bits(before, snapshot(con.lib))


def test_engine_ranks_as_the_cpu_oracle_from_the_written_file(tmp_path):
    """kge_write_type_constraints' file read by the CPU oracle: random score vectors rank to the same eight numbers as this
    engine's testHead / testTail over the device-built lists."""
    from oracle import oracle
    kg = read_kg("kg_small")
    d = str(tmp_path)
    for f in os.listdir(kg["dir"]):
        if f not in ("type_constrain.txt", "ontology_constrain.txt"):
            shutil.copy(os.path.join(kg["dir"], f), d)
    open(os.path.join(d, "ontology_constrain.txt"), "w").write("0\n")      # no classes on either side: ontology lists do not come by array
    con = build("device", kg, derive_types=True)
    _lib.check(con.lib.kge_write_type_constraints(os.path.join(d, "type_constrain.txt").encode()), con.lib)
    ev = oracle.Eval(d)
    rng = np.random.default_rng(11)
    for i in rng.choice(ev.testTotal, 5, replace=False).tolist():
        for head in (True, False):
            scores = rng.standard_normal(kg["E"]).astype(np.float32)
            got = (con.lib.testHead if head else con.lib.testTail)(i, scores.ctypes.data).contents
            assert list(got) == ev.rank(i, scores, head).tolist(), (i, head)


def test_every_evaluation_entry_point_from_arrays_equals_files(tmp_path):
    from openkeonspark_amd.TransE import TransE
    kg = read_kg("kg_small")
    d = str(tmp_path)
    for f in os.listdir(kg["dir"]):
        if f != "ontology_constrain.txt":                  # (ontology lists do not come by array: compare without classes on both sides)
            shutil.copy(os.path.join(kg["dir"], f), d)
    csr = read_type_file(os.path.join(d, "type_constrain.txt"), kg["R"])
    L = _lib.lib()

    def results(con):
        con.seed = 3
        con.set_dimension(32)
        con.set_model_and_session(TransE)
        L.kge_set_option(b"libc_rand_restart", 1)
        vh, vt, vr = kg["valid"]
        out = dict(lp=con.link_prediction()[0], rank=con.rank_triples(vh, vt, vr)[0], rel=con.relation_prediction()[0])
        ids, scores = con.top_k_tails(kg["test"][0][:16], kg["test"][2][:16], 10, filtered=True, type_constrained=True)
        out.update(topk_ids=np.asarray(ids), topk_scores=np.asarray(scores).view(np.uint32))
        tc = con.triple_classification("test")
        out.update(tc=np.array([tc[k] for k in ("tp", "tn", "fp", "fn")]), tc_acc=np.float32(tc["acc"]).view(np.uint32))
        out["valid_acc"] = np.float64(con.validation_accuracy()).view(np.uint64)
        roc = con.roc_auc("test")
        out.update(roc_auc=roc["auc"].view(np.uint64), roc_n=roc["n"])
        out["valid_mrr"] = np.float64(con.validation_link_prediction()[1]["r_filter_reci_rank"]).view(np.uint64)
        return out

    ref = Config()
    ref.set_in_path(d); ref.set_work_threads(4); ref.set_bern(1); ref.set_nbatches(7)
    ref.set_test_link_prediction(True)
    ref.init()
    want = results(ref)
    got = results(build("device", kg, type_lists=csr))
    # typed columns and classification did run (test triples of a relation without validation triples are not classified)
    assert want["lp"][:, :, 2].sum() > 0 and 0 < want["tc"].sum() <= 2 * len(kg["test"][0])
    for k in want:
        assert np.array_equal(np.asarray(want[k]), np.asarray(got[k])), k


def typed_batches(con, calls=3, B=300, n=5):
    con.set_type_constrained_sampling(True)
    seeds = np.arange(1, 5, dtype=np.uint64) * np.uint64(2654435761)
    assert con.lib.kge_set_stream_states(seeds.ctypes.data, 4) == 0
    tot = B * (1 + n)
    bh = np.zeros(tot, np.int64); bt = np.zeros(tot, np.int64); br = np.zeros(tot, np.int64); by = np.zeros(tot, np.float32)
    out = []
    for _ in range(calls):
        con.lib.sampling(bh.ctypes.data, bt.ctypes.data, br.ctypes.data, by.ctypes.data, B, n, 0)
        out.append(np.stack([bh, bt, br]).copy())
    con.set_type_constrained_sampling(False)
    return out


def test_typed_sampling_from_device_derived_lists():
    kg = read_kg("kg_small")
    host = typed_batches(build("host", kg, derive_types=True))
    dev = typed_batches(build("device", kg, derive_types=True))
    untyped = build("host", kg)
    seeds = np.arange(1, 5, dtype=np.uint64) * np.uint64(2654435761)
    assert untyped.lib.kge_set_stream_states(seeds.ctypes.data, 4) == 0
    tot = 300 * 6
    bh = np.zeros(tot, np.int64); bt = np.zeros(tot, np.int64); br = np.zeros(tot, np.int64); by = np.zeros(tot, np.float32)
    untyped.lib.sampling(bh.ctypes.data, bt.ctypes.data, br.ctypes.data, by.ctypes.data, 300, 5, 0)
    assert not np.array_equal(np.stack([bh, bt, br]), host[0])      # the lists do steer the negatives
    for a, b in zip(host, dev):
        assert np.array_equal(a, b)
