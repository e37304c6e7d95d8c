"""Evaluation from arrays and type lists without a file, on the host build: kge_import_eval_arrays against importTestFiles,
kge_set_type_lists / kge_derive_type_lists / kge_write_type_constraints against importTypeFiles and against the lists the
reference's n_n() generates (main_spark.py:209-290, restated in eval_arrays_cases.n_n_lists).  No device is needed: the arrays
are read back through kge_eval_copy, which copies from the host state where there is no GPU."""
import os
import shutil

import numpy as np
import pytest

from eval_arrays_cases import (array_config, assert_same_triples, file_config, n_n_lists, read_kg, read_type_file, snapshot,
                               type_slices)
from test_host_index import index_array
from openkeonspark_amd import _lib
from openkeonspark_amd.Config import Config

KGS = ["kg_tiny", "kg_small"]


@pytest.fixture(autouse=True)
def host_build():
    """Pin the host build whatever the box: these tests are about kg_index.cpp's side."""
    L = _lib.lib()
    _lib.check(L.kge_set_option(b"eval_index_device_min", -1), L)
    yield
    L.kge_set_option(b"eval_index_device_min", 1 << 22)


@pytest.mark.parametrize("kg_name", KGS)
def test_array_import_equals_file_import(kg_name):
    kg = read_kg(kg_name)
    want = snapshot(file_config(kg["dir"]).lib)
    csr = read_type_file(os.path.join(kg["dir"], "type_constrain.txt"), kg["R"])
    con = array_config(kg, type_lists=csr)
    got = snapshot(con.lib)
    assert want["totals"].tolist() == [len(kg["test"][0]), len(kg["valid"][0]), sum(len(kg[s][0]) for s in ("train", "valid", "test"))]
    assert (con.testTotal, con.validTotal) == (len(kg["test"][0]), len(kg["valid"][0]))
    assert_same_triples(want, got)
    assert type_slices(want) == type_slices(got)
    assert any(len(v) for v in type_slices(got)[0].values())
    # the lists come back as the CSR they went in as, each list sorted
    ho, hi, to, ti = con.type_constraints()
    assert np.array_equal(ho, csr[0]) and np.array_equal(to, csr[2])
    for off, ids, src in ((ho, hi, csr[1]), (to, ti, csr[3])):
        for q in range(kg["R"]):
            assert ids[off[q]:off[q + 1]].tolist() == sorted(src[off[q]:off[q + 1]].tolist())


@pytest.mark.parametrize("kg_name", KGS)
def test_evaluation_arrays_after_a_file_init(kg_name):
    """init() for the training set, arrays for the evaluation: the same lists as files alone."""
    kg = read_kg(kg_name)
    want = snapshot(file_config(kg["dir"]).lib)
    con = Config()
    con.set_in_path(kg["dir"]); con.set_work_threads(4)
    con.init()
    con.init_evaluation_from_arrays(kg["valid"], kg["test"])
    assert_same_triples(want, snapshot(con.lib))
    assert con.lib.kge_have_type_lists() == 0


@pytest.mark.parametrize("kg_name", KGS)
@pytest.mark.parametrize("entrance", ["files", "arrays"])
def test_derived_lists_are_n_n(kg_name, entrance):
    kg = read_kg(kg_name)
    if entrance == "files":
        con = file_config(kg["dir"])
        con.derive_type_constraints()
    else:
        con = array_config(kg, derive_types=True)
    heads, tails = n_n_lists(kg["R"], kg["train"], kg["valid"], kg["test"])
    got = snapshot(con.lib)
    assert type_slices(got) == (heads, tails)
    # back to back in relation order, a relation without triples an empty range at the running offset
    assert got["head_lef"].tolist() == np.cumsum([0] + [len(heads[q]) for q in range(kg["R"])])[:-1].tolist()
    assert got["tail_rig"].tolist() == np.cumsum([len(tails[q]) for q in range(kg["R"])]).tolist()


def test_relations_without_triples_get_empty_lists():
    kg = dict(E=6, R=4, train=([0, 1, 1], [1, 2, 2], [2, 2, 0]), valid=([3], [4], [2]), test=([], [], []))
    con = array_config(kg, derive_types=True)
    heads, tails = type_slices(snapshot(con.lib))
    assert heads == {0: [1], 1: [], 2: [0, 1, 3], 3: []} and tails == {0: [2], 1: [], 2: [1, 2, 4], 3: []}
    ho, hi, to, ti = con.type_constraints()
    assert ho.tolist() == [0, 1, 1, 4, 4] and hi.tolist() == [1, 0, 1, 3] and to.tolist() == [0, 1, 1, 4, 4] and ti.tolist() == [2, 1, 2, 4]


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """kg_small with the derived lists written in place of the committed type_constrain.txt -> (directory, heads, tails)."""
    kg = read_kg("kg_small")
    d = str(tmp_path_factory.mktemp("kg_small_derived"))
    for f in os.listdir(kg["dir"]):
        if f != "type_constrain.txt":
            shutil.copy(os.path.join(kg["dir"], f), d)
    L = _lib.lib()
    L.kge_set_option(b"eval_index_device_min", -1)
    con = Config()
    con.set_in_path(d); con.set_work_threads(4)
    con.init()
    con.init_link_prediction()
    con.derive_type_constraints(write=True)
    return (d,) + n_n_lists(kg["R"], kg["train"], kg["valid"], kg["test"])


def test_written_file_has_a_line_pair_for_every_relation(written):
    d, heads, tails = written
    lines = open(os.path.join(d, "type_constrain.txt")).read().split("\n")
    R = len(heads)
    assert lines[0] == str(R) and lines[-1] == "" and len(lines) == 2 * R + 2
    for q in range(R):
        for line, ids in ((lines[1 + 2 * q], heads[q]), (lines[2 + 2 * q], tails[q])):
            assert line == "\t".join(str(x) for x in [q, len(ids)] + ids)


def test_written_file_round_trips_through_importTypeFiles(written):
    d, heads, tails = written
    con = file_config(d)                           # importTestFiles + importTypeFiles on the written file
    assert type_slices(snapshot(con.lib)) == (heads, tails)


def test_committed_type_file_is_not_the_derived_one(written):
    """Why no test here compares against tests/golden/kg_small/type_constrain.txt."""
    kg = read_kg("kg_small")
    assert type_slices(snapshot(file_config(kg["dir"]).lib)) != (written[1], written[2])


def test_cpu_oracle_reads_the_written_file(written):
    """oracle.Eval parses the file as the reference's reader does; its typed columns on random scores are the counts over the
    derived lists, worked out here, and its untyped columns are those it gives with the committed file."""
    from oracle import oracle
    d, heads, tails = written
    kg = read_kg("kg_small")
    ev, ev0 = oracle.Eval(d), oracle.Eval(kg["dir"])
    known = set(zip(*[np.concatenate([kg[s][c] for s in ("train", "valid", "test")]).tolist() for c in (0, 1, 2)]))
    rng = np.random.default_rng(7)
    for i in rng.choice(ev.testTotal, 6, replace=False).tolist():
        h, t, r = ev.test_triple(i)
        for head in (True, False):
            scores = rng.standard_normal(kg["E"]).astype(np.float32)
            got = ev.rank(i, scores, head)
            target, lst = (h, heads[r]) if head else (t, tails[r])
            better = [j for j in lst if j != target and scores[j] < scores[target]]
            unknown = [j for j in better if ((j, t, r) if head else (h, j, r)) not in known]
            assert got[2] == len(better) and got[3] == len(unknown), (i, head)
            assert got[:2].tolist() == ev0.rank(i, scores, head)[:2].tolist()


# ---- errors ------------------------------------------------------------------------------------------------------
def test_out_of_range_ids_name_the_split_and_leave_the_old_state():
    kg = read_kg("kg_tiny")
    con = array_config(kg, derive_types=True)
    before = snapshot(con.lib)
    good = kg["valid"]
    for split, col, bad in (("valid", 0, kg["E"]), ("valid", 2, kg["R"]), ("test", 1, -1), ("test", 2, kg["R"] + 5)):
        arrs = [a.copy() for a in kg[split]]
        arrs[col][3] = bad
        with pytest.raises(_lib.KgeError, match=r"%s: id out of range at index 3" % split):
            con.init_evaluation_from_arrays(arrs if split == "valid" else good, arrs if split == "test" else kg["test"])
    after = snapshot(con.lib)
    assert_same_triples(before, after)
    assert type_slices(before) == type_slices(after)


def test_bad_type_lists_change_nothing():
    kg = read_kg("kg_tiny")
    con = array_config(kg, derive_types=True)
    before = type_slices(snapshot(con.lib))
    R, E = kg["R"], kg["E"]
    off = np.arange(R + 1, dtype=np.int64)
    ids = np.zeros(R, np.int64)
    dec = off.copy(); dec[2] = 0
    for args in ((off + 1, np.zeros(R + 1, np.int64), off, ids), (dec, ids, off, ids), (off, ids, off, ids + E),
                 (off, ids - 1, off, ids), (off[:-1], ids[:-1], off, ids)):
        with pytest.raises(_lib.KgeError):
            con.set_type_constraints(*args)
    assert type_slices(snapshot(con.lib)) == before


def test_derive_before_any_evaluation_import_is_refused():
    """The engine is one per process and keeps its evaluation lists across training imports, so "before any evaluation import"
    needs a process of its own."""
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from openkeonspark_amd.Config import Config\n"
            "from openkeonspark_amd import _lib\n"
            "con = Config(); L = con.lib\n"
            "assert L.kge_import_eval_arrays(0, None, None, None, 0, None, None, None) == -2\n"      # KGE_ERR_NO_DATASET: no training set
            "con.init_from_arrays(5, 2, [0, 1], [1, 2], [0, 1])\n"
            "assert L.kge_derive_type_lists() == -2 and 'evaluation import' in _lib.last_error(L)\n"
            "assert L.kge_eval_copy(b'all', None, 0) == -2\n"
            "print('refused')\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refused" in out.stdout, out.stderr[-2000:]


def test_no_dataset_errors():
    con = Config()
    con.init_from_arrays(5, 2, [0, 1], [1, 2], [0, 1])
    con.init_evaluation_from_arrays(([], [], []), ([], [], []))      # both splits empty is legal
    assert (con.testTotal, con.validTotal, con.lib.getTripleTotal()) == (0, 0, 2)
    with pytest.raises(_lib.KgeError):
        con.type_constraints()                                       # the import dropped whatever lists there were
    with pytest.raises(_lib.KgeError, match="in_path"):
        con.derive_type_constraints(write=True)
    con.derive_type_constraints()
    assert con.type_constraints()[1].tolist() == [0, 1]


# ---- typed sampling from lists that came by array or by derivation ----------------------------------------------------
def test_typed_sampling_after_init_from_arrays():
    kg = read_kg("kg_small")
    con = Config()
    con.set_work_threads(4)
    con.init_from_arrays(kg["E"], kg["R"], *kg["train"])
    with pytest.raises(_lib.KgeError, match="init_from_arrays.*init_evaluation_from_arrays"):
        con.set_type_constrained_sampling(True)
    con.set_type_constrained_sampling(False)
    con.init_evaluation_from_arrays(kg["valid"], kg["test"], derive_types=True)
    con.set_type_constrained_sampling(True)
    assert con.lib.kge_typed_sampling() == 1


def test_typed_index_from_derived_lists_equals_the_written_file(written):
    kg = read_kg("kg_small")
    names = (("type_tails", None), ("type_heads", None), ("type_bounds", 4), ("typed_pos_hr", None), ("typed_pos_tr", None), ("typed_len", 2))
    con = Config()
    con.set_work_threads(4)
    con.init_from_arrays(kg["E"], kg["R"], *kg["train"])
    con.init_evaluation_from_arrays(kg["valid"], kg["test"], derive_types=True)
    con.set_type_constrained_sampling(True)
    got = {n: index_array(con.lib, n, np.int32, c) for n, c in names}
    ref = Config()
    ref.set_in_path(written[0]); ref.set_work_threads(4)
    ref.set_type_constrained_sampling(True)
    ref.init()                                     # importTypeFiles on the written file
    want = {n: index_array(ref.lib, n, np.int32, c) for n, c in names}
    assert len(want["type_tails"]) > 0
    for n in want:
        assert np.array_equal(got[n], want[n]), n
    # explicit lists (the file's, as CSR) serve as well, and a later evaluation import drops them again
    con.init_evaluation_from_arrays(kg["valid"], kg["test"], type_lists=read_type_file(os.path.join(written[0], "type_constrain.txt"), kg["R"]))
    for n in want:
        assert np.array_equal(index_array(con.lib, n, np.int32, dict(names)[n]), want[n]), n
    con.set_type_constrained_sampling(False)
    con.init_evaluation_from_arrays(kg["valid"], kg["test"])
    with pytest.raises(_lib.KgeError, match="init_from_arrays"):
        con.set_type_constrained_sampling(True)
