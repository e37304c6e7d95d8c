"""CPU-side checks of the engine library: it loads, exports the whole C ABI, and its host loader /
filter index agrees with the reference-pinned oracle.  No compute entry point is called here."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import oracle
from openkeonspark_amd import _lib
from openkeonspark_amd.Config import Config


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "kge_mi355.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", text)
    skip = {"defined", "sizeof"}
    return sorted({n for n in names if n not in skip and not n.isupper()})


def test_library_exports_every_declared_symbol():
    L = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    assert "sampling" in syms and "kge_forward_backward" in syms and len(syms) >= 30
    for s in syms:
        assert hasattr(L, s), s


def test_base_so_hot_path_names_present():
    # the names Config.py:30-31,160-170,347 binds
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in ["setInPath", "setOutPath", "setWorkThreads", "getWorkThreads", "setBern", "randReset", "importTrainFiles",
              "getEntityTotal", "getRelationTotal", "getTripleTotal", "getTrainTotal", "getTrainTotal_", "getTestTotal",
              "getValidTotal", "getBatchTotal", "sampling"]:
        assert hasattr(L, s), s


def index_array(L, name, dtype, cols=None):
    nbytes = L.kge_index_copy(name.encode(), None, 0)
    assert nbytes >= 0
    a = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
    L.kge_index_copy(name.encode(), a.ctypes.data, nbytes)
    return a.reshape(-1, cols) if cols else a


@pytest.mark.parametrize("kg_name", ["kg_tiny", "kg_small", "kg_incr"])
def test_host_index_matches_oracle(kg_name):
    con = Config()
    con.set_in_path(os.path.join(GOLDEN, kg_name))
    con.set_work_threads(3)
    con.init()
    kg = oracle.KG(os.path.join(GOLDEN, kg_name), work_threads=3)
    z = np.load(os.path.join(GOLDEN, "%s_W3_bern0.npz" % kg_name))
    L = con.lib
    assert [L.getEntityTotal(), L.getRelationTotal(), L.getTrainTotal(), L.getTrainTotal_(), L.getBatchTotal()] \
        == z["totals"].tolist()
    assert con.trainTotal == kg.trainTotal_ and con.bt == kg.batchTotal
    assert np.array_equal(index_array(L, "tails_hr", np.int32), z["by_head"][:, 2])
    assert np.array_equal(index_array(L, "heads_tr", np.int32), z["by_tail"][:, 0])
    assert np.array_equal(index_array(L, "rels_ht", np.int32), z["by_rel"][:, 1])
    assert index_array(L, "left_mean", np.float32).tobytes() == z["left_mean"].tobytes()
    assert index_array(L, "right_mean", np.float32).tobytes() == z["right_mean"].tobytes()
    # every file-order triple's groups contain exactly the known tails / heads / relations
    pos = index_array(L, "pos", np.int32, 4)
    grp = index_array(L, "grp", np.int32, 4)
    ht = index_array(L, "ht", np.int32, 2)
    tails, heads, rels = (index_array(L, n, np.int32) for n in ("tails_hr", "heads_tr", "rels_ht"))
    uniq = {(int(a), int(b), int(c)) for a, b, c in z["by_head"]}  # (h, r, t)
    for i in range(0, len(pos), max(1, len(pos) // 200)):
        h, t, r, _ = pos[i]
        assert set(tails[grp[i, 0]:grp[i, 0] + grp[i, 1]]) == {tt for (hh, rr, tt) in uniq if hh == h and rr == r}
        assert set(heads[grp[i, 2]:grp[i, 2] + grp[i, 3]]) == {hh for (hh, rr, tt) in uniq if tt == t and rr == r}
        assert set(rels[ht[i, 0]:ht[i, 0] + ht[i, 1]]) == {rr for (hh, rr, tt) in uniq if hh == h and tt == t}
    # Base.cpp:117 probability, float arithmetic as written there
    lm, rm = z["left_mean"], z["right_mean"]
    with np.errstate(invalid="ignore"):
        want = (np.float32(1000) * rm) / (rm + lm)
    got = index_array(L, "bern_prob", np.float32)
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]) and np.isnan(got[~ok]).all()


def test_missing_directory_is_reported_not_fatal():
    con = Config()
    con.set_in_path("/nonexistent/dir")
    with pytest.raises(_lib.KgeError, match="does not exist"):  # reference prints the same text (Reader.h:36-39)
        con.init()


def test_out_of_range_ids_are_rejected():
    con = Config()
    with pytest.raises(_lib.KgeError, match="out of range"):
        con.init_from_arrays(5, 2, [0, 7], [1, 2], [0, 1])


def test_mini_batch_rule_and_buffers():
    # Config.py:189-210: auto batch = total divided by 10 until <= 9999; nbatches = int(total / batch)
    con = Config()
    h = np.arange(27211) % 50
    con.init_from_arrays(50, 3, h, (h + 1) % 50, h % 3)
    assert (con.batch_size, con.nbatches) == (2721, 10)
    con2 = Config()
    con2.set_nbatches(4)
    con2.set_ent_neg_rate(25)
    con2.init_from_arrays(50, 3, h, (h + 1) % 50, h % 3)
    assert con2.batch_size == 6802 and con2.batch_seq_size == 6802 * 26
    assert con2.batch_h.dtype == np.int64 and con2.batch_y.dtype == np.float32 and len(con2.batch_h) == 6802 * 26


def test_slice_positions_tile_the_batch():
    from openkeonspark_amd.parallel import slice_positions, thread_range
    con = Config()
    for W in (1, 3, 8, 16):
        con.set_work_threads(W)
        con.lib.setWorkThreads(W)
        for B in (1, 7, 50, 64, 2721, 68028):
            covered = 0
            for lo in range(W):
                first = ctypes.c_int64()
                n = con.lib.kge_slice_positions(B, lo, lo + 1, ctypes.byref(first))
                assert (first.value, n) == slice_positions(B, W, lo, lo + 1)
                if n:
                    assert first.value == covered
                covered += n
            assert covered == B
            for G in (1, 2, 4, 8):
                if W % G:
                    continue
                tot = 0
                for g in range(G):
                    a, b = thread_range(g, G, W)
                    f, n = slice_positions(B, W, a, b)
                    assert n == 0 or f == tot
                    tot += n
                assert tot == B


def test_model_batch_views_follow_the_reference_layout():
    """Model.get_*_instance / labels (Model.py:10-53): negative k of positive b sits at B*(k+1)+b in the flat batch and at
    [b, k] of the in-batch view."""
    from openkeonspark_amd.Model import Model

    class Cfg:
        batch_size, negative_ent, negative_rel = 4, 2, 1
        batch_seq_size = 4 * (1 + 2 + 1)
        batch_h = np.arange(16) * 10
        batch_t = np.arange(16) * 10 + 1
        batch_r = np.arange(16) * 10 + 2
        batch_y = np.where(np.arange(16) < 4, 1.0, -1.0).astype(np.float32)

    m = Model.__new__(Model)
    m.config = Cfg
    ph, pt, pr = m.get_positive_instance()
    assert ph.shape == (4, 1) and ph[:, 0].tolist() == [0, 10, 20, 30] and pr[2, 0] == 22
    nh, nt, nr = m.get_negative_instance()
    assert nh.shape == (4, 3)
    for b in range(4):
        for k in range(3):
            assert nh[b, k] == Cfg.batch_h[4 * (k + 1) + b] and nt[b, k] == Cfg.batch_t[4 * (k + 1) + b]
    assert m.get_negative_instance(in_batch=False)[0].tolist() == Cfg.batch_h[4:].tolist()
    assert m.get_positive_labels().ravel().tolist() == [1.0] * 4 and (m.get_negative_labels() == -1).all()
    ah, _, _ = m.get_all_instance(in_batch=True)
    assert ah.shape == (4, 4) and ah[1].tolist() == [10, 50, 90, 130]
    assert m.get_all_labels().shape == (16,) and m.get_all_instance()[2] is Cfg.batch_r


def test_pair_count_path_selection_rule():
    """kge_pair_path_active (include/kge_mi355.h): which TransH / TransD steps take the pair-count path -- host logic only, no
    device needed: widths that are multiples of 4 up to 256, at most 63 negatives, from 5 (TransH) / 3 (TransD) negatives and
    65 536 entity-side rows per step, ent_total*rel_total below 2^31."""
    from openkeonspark_amd import _lib
    L = _lib.lib()

    def active(model, E, R, D, B, n):
        d = _lib.ModelDesc(model, 0, E, R, D, D, 1.0, 0)
        return L.kge_pair_path_active(ctypes.byref(d), B, n)

    H, Dm, Em, Rm = _lib.TRANSH, _lib.TRANSD, _lib.TRANSE, _lib.TRANSR
    assert active(H, 40943, 11, 200, 43417, 25) == 1 and active(Dm, 14541, 237, 200, 34014, 25) == 1
    assert active(H, 40943, 11, 200, 43417, 4) == 0 and active(H, 40943, 11, 200, 43417, 5) == 1      # measured cross-over
    assert active(Dm, 14541, 237, 200, 34014, 2) == 0 and active(Dm, 14541, 237, 200, 34014, 3) == 1
    assert active(H, 40943, 11, 200, 2000, 25) == 0                                                    # 54 000 rows: a small step
    assert active(H, 40943, 11, 202, 43417, 25) == 0 and active(H, 40943, 11, 260, 43417, 25) == 0     # width
    assert active(H, 40943, 11, 200, 43417, 64) == 0                                                    # int8 range of the sums
    assert active(Em, 14541, 237, 200, 34014, 25) == 0 and active(Rm, 14541, 237, 200, 34014, 25) == 0
    assert active(H, 3_000_000, 1000, 200, 43417, 25) == 0                                             # keys must fit an int32
    assert active(H, 14951, 1345, 200, 43417, 25) == 1                                                  # 20 M keys: radix-sort ordering
    L.kge_set_option(b"pair_counts", 0)
    try:
        assert active(H, 40943, 11, 200, 43417, 25) == 0
    finally:
        L.kge_set_option(b"pair_counts", 1)


def test_transr_group_layout_selection_rule():
    """kge_transr_group_layout_active (include/kge_mi355.h): which sampler-shaped TransR steps take the group layout -- host
    logic only: dims that are multiples of 4 up to 208, 2 + n <= 16, the positive's matrix for every negative, (R + 1) * 4
    relation bins at most 4096, and (transr_groups = 1) at least 64 rows per relation; the launcher asks the same function."""
    from openkeonspark_amd import _lib
    L = _lib.lib()

    def active(model, R, De, Dr, B, n, nr=0):
        d = _lib.ModelDesc(model, nr, 14541, R, De, Dr, 1.0, 0)
        return L.kge_transr_group_layout_active(ctypes.byref(d), B, n)

    Rm = _lib.TRANSR
    assert active(Rm, 237, 200, 200, 34014, 1) == 1                                          # config #4 at nbatches 8
    assert active(Rm, 237, 200, 200, 2721, 1) == 0                                           # the reference's batch: 34 rows per relation
    assert active(Rm, 237, 200, 200, 34014, 14) == 1 and active(Rm, 237, 200, 200, 34014, 15) == 0     # U = 16 fits a sub-tile
    assert active(Rm, 237, 200, 200, 34014, 1, nr=1) == 0                                    # a negative's own matrix
    assert active(Rm, 237, 202, 200, 34014, 1) == 0 and active(Rm, 237, 200, 212, 34014, 1) == 0
    assert active(Rm, 237, 208, 4, 34014, 1) == 1
    assert active(Rm, 237, 200, 200, 0, 1) == 0
    assert active(_lib.TRANSE, 237, 200, 200, 34014, 1) == 0 and active(_lib.TRANSH, 237, 200, 200, 34014, 1) == 0
    L.kge_set_option(b"transr_groups", 2)
    try:
        assert active(Rm, 237, 200, 200, 300, 1) == 1
        assert active(Rm, 1023, 64, 100, 300, 1) == 1 and active(Rm, 1024, 64, 100, 300, 1) == 0   # (R + 1) * 4 <= 4096
        for opt, val in ((b"transr_bf16x3", 0), (b"transr_v1", 1), (b"counts_force_sort", 1)):
            L.kge_set_option(opt, val)
            try:
                assert active(Rm, 237, 200, 200, 34014, 1) == 0, opt
            finally:
                L.kge_set_option(opt, {b"transr_bf16x3": 1}.get(opt, 0))
    finally:
        L.kge_set_option(b"transr_groups", 1)
    L.kge_set_option(b"transr_groups", 0)
    try:
        assert active(Rm, 237, 200, 200, 34014, 1) == 0
    finally:
        L.kge_set_option(b"transr_groups", 1)


def test_transe_relation_copies_rule():
    """kge_transe_relation_copies (include/kge_mi355.h): the virtual copies of the relation rows a sign-count step sorts its
    records over -- host logic only: 1 below 4096 groups, else option counts_krel (rounded down to a power of two, at most
    64), halved while copies * R > 2 (E + R); forward_counts_impl asks the same function."""
    from openkeonspark_amd import _lib
    L = _lib.lib()

    def copies(E, R, B, model=_lib.TRANSE, D=16):
        d = _lib.ModelDesc(model, 0, E, R, D, D, 1.0, 0)
        return L.kge_transe_relation_copies(ctypes.byref(d), B)

    assert copies(61, 4, 4095) == 1 and copies(61, 4, 4096) == 4 and copies(61, 4, 4097) == 4     # the threshold
    assert copies(14541, 237, 34014) == 4 and copies(14541, 237, 300) == 1
    assert copies(61, 0, 4096) == 1                                                                 # no relation rows
    # halving: 4 * 4 = 16 <= 2 * 65 keeps 4; 4 * 40 = 160 > 2 * 50 = 100 halves to 2 (80 <= 100)
    assert copies(61, 4, 4096) == 4 and copies(10, 40, 4096) == 2
    assert copies(1, 40, 4096) == 2 and copies(1, 400, 4096) == 2 and copies(0, 40, 4096) == 2    # k R <= 2 R always holds at k = 2
    try:
        for value, want in ((1, 1), (2, 2), (4, 4), (8, 8), (64, 64), (6, 4), (100, 64), (0, 1)):
            L.kge_set_option(b"counts_krel", value)
            assert copies(2000, 4, 4096) == want, (value, want)
            assert copies(2000, 4, 4095) == 1
        L.kge_set_option(b"counts_krel", 64)
        assert copies(61, 4, 4096) == 32 and copies(10, 40, 4096) == 2                              # 32 * 4 = 128 <= 130
    finally:
        L.kge_set_option(b"counts_krel", 4)


def test_float_records_chunk_length_rule():
    """kge_float_records_chunk_len: records per team of the float-record segmented sum -- 16, 32 from 2^18 records, 64 from 2^20."""
    from openkeonspark_amd import _lib
    L = _lib.lib()
    assert [L.kge_float_records_chunk_len(n) for n in (0, 1, (1 << 18) - 1, 1 << 18, (1 << 20) - 1, 1 << 20, 1 << 31)] \
        == [16, 16, 16, 32, 32, 64, 64]
