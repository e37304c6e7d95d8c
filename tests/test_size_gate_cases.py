"""The cases of tests/test_gpu_size_gates.py, built without a GPU: every batch is tie-free after redrawing at most 5 % of its
groups, keeps the reference's batch layout, and -- asked through the engine's host-only queries -- crosses the size gate it is
meant for.  Each test prints its case's redraw share and the gate value the engine reports."""
import ctypes

import numpy as np
import pytest

import size_gate_cases as sg
from openkeonspark_amd import _lib


def desc(model, E, R, D, nr=0):
    return _lib.ModelDesc({"transe": _lib.TRANSE, "transh": _lib.TRANSH, "transd": _lib.TRANSD}[model], nr, E, R, D, D, 1.0, 0)


def copies(E, R, D, B, krel=4, nr=0):
    L = _lib.lib()
    L.kge_set_option(b"counts_krel", krel)
    try:
        return L.kge_transe_relation_copies(ctypes.byref(desc("transe", E, R, D, nr)), B)
    finally:
        L.kge_set_option(b"counts_krel", 4)


@pytest.mark.parametrize("E,R,D,n,B,krel,want_copies", sg.EXACT_CASES + sg.EXACT_SECOND_TRIP)
def test_exact_count_cases(E, R, D, n, B, krel, want_copies):
    from torch_ref import near_kink_rows
    c = sg.exact_case(E, R, D, n, B)
    bh, bt, br = c["batch"]
    got = copies(E, R, D, B, krel)
    print("exact E=%d R=%d D=%d n=%d B=%d: redrawn %.3f %% of the groups, relation copies %d" % (E, R, D, n, B, 100 * c["share"], got))
    assert c["share"] <= sg.MAX_REDRAW_SHARE and got == want_copies
    sg.check_layout(bh, bt, br, B, n, 0, E, R, sampler_shaped=True)
    assert near_kink_rows("transe", c["params"], bh, bt, br, B, n, D, D, tol=sg.KINK)[1] == 0
    assert c["want"].shape == (E + R, D) and not c["want"][:E].sum(0).any() and np.abs(c["want"]).sum() > 0
    if B == sg.SECOND_TRIP_B:
        assert D <= 64 and B > sg.MAX_LOSS_BLOCKS * 256 // 16        # a 16-lane team takes a second group


@pytest.mark.parametrize("n,nr,foreign,D", sg.RELNEG_CASES)
def test_relation_negative_cases(n, nr, foreign, D):
    c = sg.relneg_case(n, nr, foreign, D)
    got = copies(sg.RELNEG_E, sg.RELNEG_R, D, sg.RELNEG_B, nr=nr)
    print("relneg n=%d nr=%d foreign=%.1f D=%d: redrawn %.3f %% of the groups, relation copies %d" % (n, nr, foreign, D, 100 * c["share"], got))
    assert c["share"] <= sg.MAX_REDRAW_SHARE and got == 4
    sg.check_layout(*c["batch"], sg.RELNEG_B, n, nr, sg.RELNEG_E, sg.RELNEG_R, sampler_shaped=False)
    r = c["batch"][2].reshape(1 + n + nr, sg.RELNEG_B)
    assert (r[1 + n:] != r[:1]).any()                      # relation negatives with another relation's row
    if foreign:
        assert len(sg.foreign_groups(*(x[:sg.RELNEG_B * (1 + n)] for x in c["batch"]), sg.RELNEG_B, n)) > 0


def test_fused_graph_gives_batches_with_relation_copies():
    from openkeonspark_amd.Config import Config
    E, R, h, t, r = sg.fused_graph()
    con = Config()
    con.set_nbatches(sg.FUSED_NBATCHES)
    con.set_ent_neg_rate(sg.FUSED_NEG)
    con.init_from_arrays(E, R, h, t, r)
    got = [copies(E, R, D, con.batch_size) for D in (16, 100)]
    print("fused graph: batch size %d, relation copies %s" % (con.batch_size, got))
    assert con.batch_size >= 4096 and got == [4, 4]


@pytest.mark.parametrize("model,D,B,chunk", sg.CHUNK_CASES)
def test_chunk_length_cases(model, D, B, chunk):
    n = sg.CHUNK_NEG[model]
    c = sg.chunk_case(model, D, B)
    records = B * sg.RECORD_SLOTS[model](n)
    got = _lib.lib().kge_float_records_chunk_len(records)
    print("chunk %s D=%d B=%d: %d records, chunk length %d, redrawn %.3f %% of the groups" % (model, D, B, records, got, 100 * c["share"]))
    assert c["share"] <= sg.MAX_REDRAW_SHARE and got == chunk
    assert abs(records - (1 << 18 if chunk < 64 else 1 << 20)) <= 16
    sg.check_layout(*c["batch"], B, n, 0, sg.CHUNK_E, sg.CHUNK_R, sampler_shaped=False)
    assert np.bincount(c["batch"][2][:B], minlength=sg.CHUNK_R).min() > 64 * chunk      # hub runs that span many chunks


@pytest.mark.parametrize("model,D", sg.PAIR_TRIP_CASES + [("transh", 16)])
def test_second_trip_cases(model, D):
    pair = (model, D) in sg.PAIR_TRIP_CASES               # (transh, 16): the atomic path's case, no foreign negatives
    B, first = sg.SECOND_TRIP_B, sg.MAX_LOSS_BLOCKS * 256 // 16
    c = sg.trip_case(model, D, 0.02 if pair else 0.0)
    bh, bt, br = c["batch"]
    print("second trip %s D=%d: redrawn %.3f %% of the groups" % (model, D, 100 * c["share"]))
    assert c["share"] <= sg.MAX_REDRAW_SHARE and B > first
    sg.check_layout(bh, bt, br, B, 1, 0, sg.TRIP_E, sg.TRIP_R, sampler_shaped=False)
    if not pair:
        return
    L = _lib.lib()
    L.kge_set_option(b"pair_counts_min_neg", 1)
    L.kge_set_option(b"float_records_min", 0)
    try:
        assert L.kge_pair_path_active(ctypes.byref(desc(model, sg.TRIP_E, sg.TRIP_R, D)), B, 1) == 1
    finally:
        L.kge_set_option(b"pair_counts_min_neg", 0)
        L.kge_set_option(b"float_records_min", 1 << 16)
    foreign = sg.foreign_groups(bh, bt, br, B, 1)
    hm = c["orc"].hinge_margins(bh, bt, br, B, 1)[:, 0]
    shaped = np.setdiff1d(np.arange(first, B), foreign)
    assert (foreign >= first).any() and (hm[shaped] < 0).any() and (hm[shaped] > 0).any()
    assert np.abs(hm).min() > sg.HINGE_TIE


def test_fp64_summed_oracle_gradient_converges_where_the_sequential_sum_does_not():
    """size_gate_cases.oracle_grad at 2^18 - 16 records: 32 and 64 groups per slice agree to 2e-6 of each table's largest
    element, the entity rows of the oracle's own sequential fp32 sum agree with them as well, and its five relation rows (up to
    46 000 contributions each) do not -- which is why these cases take the sliced form as their reference."""
    model, D, B = "transe", 8, 16383
    c = sg.chunk_case(model, D, B)
    n = sg.CHUNK_NEG[model]
    _, seq = c["orc"].grad(*c["batch"], B, n)
    _, g64 = sg.oracle_grad(c["orc"], *c["batch"], B, n, groups=64)
    err = {}
    for k, g32 in c["grads"].items():
        scale = np.abs(g32).max()
        err[k] = (np.abs(seq[k] - g32).max() / scale, np.abs(g64[k] - g32).max() / scale)
        assert err[k][1] <= 2e-6, (k, err[k])
    print("oracle gradient, (sequential fp32, 64 groups per slice) against 32 groups per slice: %s" % err)
    assert err["ent_embeddings"][0] <= 2e-6 and err["rel_embeddings"][0] > 1e-5


def test_vectorised_sign_counts_equal_the_loop():
    from oracle import oracle
    from test_gpu_models import numpy_sign_counts, rand_batch
    E, R, D, B, n = 61, 4, 16, 300, 25
    rng = np.random.default_rng(5)
    params = oracle.init_params(oracle.TRANSE, E, R, D, D, seed=2)
    bh, bt, br = rand_batch(rng, E, R, B, n, 0, distinct=True)
    want = numpy_sign_counts(params, bh, bt, br, B, n, 1.0)
    assert np.array_equal(sg.numpy_sign_counts(params, bh, bt, br, B, n, 1.0), want) and np.abs(want).sum() > 0
    bh, bt, br = rand_batch(rng, E, R, B, 3, 2, foreign=0.3)                 # relation negatives, arbitrary negatives
    assert np.array_equal(sg.numpy_sign_counts(params, bh, bt, br, B, 5, 0.5), numpy_sign_counts(params, bh, bt, br, B, 5, 0.5))
