"""Type-constrained sampling, the parts that need no GPU: the Python restatement of the batch draw is the reference's sampler
(it reproduces the committed fixtures), the typed index the library builds on the host equals the numpy construction, and
the setter's errors."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from openkeonspark_amd import _lib
from openkeonspark_amd.Config import Config

import typed_sampler_cases as tc


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    return tc.write_crafted(str(tmp_path_factory.mktemp("kg_typed_crafted")))


@pytest.fixture(scope="module")
def tiny():
    return tc.KG(os.path.join(GOLDEN, "kg_tiny"))


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("bern", [0, 1])
def test_untyped_restatement_reproduces_the_reference_fixtures(tiny, W, bern):
    z = np.load(os.path.join(GOLDEN, "kg_tiny_W%d_bern%d.npz" % (W, bern)))
    states = [int(x) for x in z["seeds"]]
    for si, (B, n, nr) in enumerate(tc.GRID_SHAPE):
        for c in range(tc.CALLS):
            h, t, r, _ = tc.sample_batch(tiny, states, B, n, nr, bern, typed=False)
            ref = z["s%d_c%d" % (si, c)]
            assert np.array_equal(h, ref[0]) and np.array_equal(t, ref[1]) and np.array_equal(r, ref[2]), (si, c)
    assert states == [int(x) for x in z["final_states"]]


def _index_array(L, name, cols=None):
    nbytes = _lib.check(L.kge_index_copy(name.encode(), None, 0), L)
    a = np.zeros(nbytes // 4, np.int32)
    L.kge_index_copy(name.encode(), a.ctypes.data, nbytes)
    return a.reshape(-1, cols) if cols else a


def _typed_config(path, on=True):
    con = Config()
    con.set_in_path(path)
    con.set_work_threads(3)
    con.set_type_constrained_sampling(on)
    con.init()
    return con


@pytest.mark.parametrize("which", ["crafted", "tiny"])
def test_typed_index_equals_the_numpy_construction(which, crafted, tiny):
    kg = crafted if which == "crafted" else tiny
    con = _typed_config(kg.path)
    try:
        assert con.lib.kge_typed_sampling() == 1
        want = tc.typed_index(kg)
        for name, cols in (("type_tails", None), ("type_heads", None), ("type_bounds", 4), ("typed_pos_hr", None),
                           ("typed_pos_tr", None), ("typed_len", 2)):
            got = _index_array(con.lib, name, cols)
            assert got.shape == want[name].shape and np.array_equal(got, want[name]), name
        # the position lists share the offsets of tails_hr / heads_tr: a group's positions fit its slots
        grp = _index_array(con.lib, "grp", 4)
        tl = want["typed_len"]
        assert (tl[:, 0] <= grp[:, 1]).all() and (tl[:, 1] <= grp[:, 3]).all()
    finally:
        con.set_type_constrained_sampling(False)
    assert con.lib.kge_typed_sampling() == 0


def test_setter_needs_a_type_file(tmp_path, crafted):
    d = str(tmp_path / "kg_untyped")
    os.makedirs(d)
    for name in ("entity2id.txt", "relation2id.txt", "train2id.txt"):
        with open(os.path.join(crafted.path, name)) as src, open(os.path.join(d, name), "w") as dst:
            dst.write(src.read())
    con = Config()
    con.set_in_path(d)
    con.set_type_constrained_sampling(True)
    with pytest.raises(_lib.KgeError, match="type_constrain.txt"):
        con.init()
    # after init(), too; and the C call says why when no type file was ever imported for this dataset
    con = Config()
    con.set_in_path(d)
    con.init()
    with pytest.raises(_lib.KgeError, match="type_constrain.txt"):
        con.set_type_constrained_sampling(True)
    con.lib.importTestFiles()       # (drops any type lists an earlier test imported; the files it wants are missing here)
    con.lib.kge_clear_error()
    assert con.lib.kge_set_typed_sampling(1) < 0 and "no type file imported" in _lib.last_error(con.lib)
    con.lib.kge_clear_error()
    assert con.lib.kge_typed_sampling() == 0


def test_init_from_arrays_has_no_type_file():
    con = Config()
    con.set_type_constrained_sampling(True)
    with pytest.raises(_lib.KgeError, match="init_from_arrays"):
        con.init_from_arrays(5, 2, [0, 1], [1, 2], [0, 1])
    con = Config()
    con.init_from_arrays(5, 2, [0, 1], [1, 2], [0, 1])
    assert con.lib.kge_typed_sampling() == 0
    with pytest.raises(_lib.KgeError, match="init_from_arrays"):
        con.set_type_constrained_sampling(True)


def test_a_later_config_starts_untyped(crafted):
    con = _typed_config(crafted.path)
    assert con.lib.kge_typed_sampling() == 1
    con2 = _typed_config(crafted.path, on=False)
    assert con2.lib.kge_typed_sampling() == 0
