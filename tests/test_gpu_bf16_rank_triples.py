"""kge_rank_triples_bf16 (include/kge_mi355.h, "Evaluation on bf16 tables"): all [n][2][4] counts of kge_rank_triples on the widened
tables, from the stored bf16 rows, with no candidate table -- one width per rung of csrc/team_shape.hpp, E = 517 (a ragged last
round at every TEAMS * U), R = 5, n = 37 triples (no multiple of the 16 / 8 / 4 requests of a block, mixed relations, duplicates),
tail side alone and both sides, one slice and three.  Family (a): normal draws with the rows a norm or a compare can trip on.
Family (b): tables of +-1, where a candidate's score differs from the true triple's by rounding order only -- a contracted
product, or a lane's 1 / |x| that is not the fp32 kernel's, moves counts."""
import os

import numpy as np
import pytest

import bf16_eval_rig as rig
import bf16_full_eval_rig as full

pytestmark = pytest.mark.gpu

E, N = 517, 37
WIDTHS = rig.MULTIPLE_OF_8_PER_RUNG


def device_triples():
    return tuple(rig.dev(x, np.int32) for x in full.triples(E, N))


def compare(tabs):
    """Both entry points at test_head 0 / 1 and rank_slices 1 / 3 -> the counts at test_head = 1 (equal everywhere)."""
    h, t, r = device_triples()
    both = None
    for test_head in (0, 1):
        rc32, want = full.rank_triples(tabs, h, t, r, test_head, bf16=False)
        assert rc32 == 0
        for slices in (1, 3):
            with full.Options(rank_slices=slices):
                rc, got = full.rank_triples(tabs, h, t, r, test_head)
            assert rc == 0, (test_head, slices, rc)
            assert np.array_equal(got, want), (test_head, slices, full.first_diff(got, want))
            assert (got >= 0).all()                                    # every element written
            if not test_head:
                assert not got[:, 1].any()
        both = want
    return both


@pytest.mark.parametrize("D", WIDTHS)
def test_counts_are_the_fp32_kernels_on_the_widened_tables(D):
    con = full.import_graph(E)
    tabs, rows = full.special_tables(E, D, N)
    counts = compare(tabs)
    assert counts[:, :, 0].any()
    # the filter and the type lists were searched: some known candidates and some typed ones lay below their true triple
    assert counts[:, :, 1].any() and (counts[:, :, 1] < counts[:, :, 0]).any() and counts[:, :, 2].any() and counts[:, :, 3].any()
    # duplicates rank alike
    assert np.array_equal(counts[N - 1], counts[0]) and np.array_equal(counts[N // 2], counts[5])
    del con


@pytest.mark.parametrize("D", (24, 40))
def test_near_tie_tables_where_only_the_rounding_order_separates_scores(D):
    con = full.import_graph(E)
    tabs = full.tie_tables(E, D)
    h, t, r = full.triples(E, N)
    close = full.near_ties(tabs, h, t, r)
    print("D = %d: %d (triple, side, candidate) with unlike rows within 4 float32 ulps of the true triple's score" % (D, close))
    assert close >= 1000                 # the condition under which equal counts say something about the last bits
    counts = compare(tabs)
    assert counts[:, :, 0].any()
    del con


def test_errors_are_the_fp32_calls_and_leave_the_counts_untouched(tmp_path):
    import torch
    con = full.import_graph(E)
    D = 24
    tabs, _ = full.special_tables(E, D, N)
    h, t, r = device_triples()
    counts = torch.full((N, 2, 4), full.FILL, dtype=torch.int64, device="cuda")
    untouched = lambda: bool((counts == full.FILL).all().item())
    cases = [dict(h=None), dict(t=None), dict(r=None), dict(n=-1)]

    def call(bf16, h=h, t=t, r=r, **kw):
        return full.rank_triples(tabs, h, t, r, 1, bf16=bf16, counts=counts, **kw)[0]
    for kw in cases:
        assert call(True, **kw) == call(False, **kw) == rig.KGE_ERR_BAD_ARG and untouched(), kw
    for kw in (dict(ent=None), dict(rel=None)):
        assert call(True, **kw) == rig.KGE_ERR_BAD_ARG and untouched(), kw
    # n == 0: arguments and files only
    assert call(True, n=0) == call(False, n=0) == 0 and untouched()
    # a relation id out of range is found after the ids have come to the host
    bad_r = r.clone(); bad_r[7] = full.R
    assert call(True, r=bad_r) == call(False, r=bad_r) == rig.KGE_ERR_BAD_ARG and untouched()
    # outside kge_bf16_eval_supported
    for desc in (rig.desc(E, full.R, 12), rig.desc(E, full.R, 1032), rig.desc(E, full.R, D, model=1), rig.desc(E, full.R, D, 8)):
        assert call(True, d=desc) == rig.KGE_ERR_UNSUPPORTED and untouched(), (desc.model, desc.ent_dim)
    # before importTestFiles (a failed import leaves the library without evaluation lists)
    empty = tmp_path / "train_only"
    os.makedirs(str(empty))
    con.lib.setInPath((str(empty) + "/").encode())
    con.lib.kge_clear_error()
    con.lib.importTestFiles()
    con.lib.kge_clear_error()
    for n in (N, 0):
        assert call(True, n=n) == call(False, n=n) == rig.KGE_ERR_NO_DATASET and untouched(), n
    del con
