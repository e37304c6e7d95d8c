"""The branches of the training step that the engine chooses by the SIZE of the step, at the smallest shapes that reach them
(tests/size_gate_cases.py; tests/test_size_gate_cases.py builds the same cases on the CPU):

  * relation-row copies of the TransE sign-count path, from 4096 groups on (csrc/transe_counts.hip transe_relation_copies):
    group b keys its relation records to virtual row E + (b & (copies - 1)) R + r, and segsum_kernel / segapply_kernel fold
    the copies back;
  * chunk lengths 32 and 64 of the float-record segmented sum, from 2^18 / 2^20 records (float_records_chunk_len);
  * the second trip of the grid-capped emit and forward/backward kernels: the grid is capped at kMaxLossBlocks = 4096
    workgroups of 256 / L teams, so a 16-lane team takes a second group from n_pos > 65 536 on.

Every test first asserts, through the engine's host-only queries, that its shape crosses the gate.  Widths stay tiny so that
records and oracle time stay small.  Tolerances are those of tests/test_gpu_models.py, imported."""
import ctypes

import numpy as np
import pytest

import size_gate_cases as sg
from conftest import parity_report
from oracle import oracle
from test_gpu_fused_counts import engine, state
from test_gpu_models import (EXACT_COUNT_ROWS_BOUND, RTOL, SIGN_FLIP_ROWS_BOUND, check_gradients_with_kinks, make_engine)

pytestmark = pytest.mark.gpu


def lib():
    from openkeonspark_amd import _lib
    return _lib.lib()


def device_batch(batch):
    import torch
    return torch.from_numpy(np.stack(batch).astype(np.int32)).cuda()


def exact_count_image(case, sort, with_loss=False):
    """forward_counts on the case's batch: the int32 image equals the definition's integer sums (rows differing <=
    EXACT_COUNT_ROWS_BOUND); the image is read and re-zeroed as test_transe_sign_counts_are_the_exact_integer_sums does."""
    E, R, D, n, B, krel, want_copies = case
    L = lib()
    c = sg.exact_case(E, R, D, n, B)
    L.kge_set_option(b"counts_force_sort", sort)
    L.kge_set_option(b"counts_krel", krel)
    try:
        con = make_engine("transe", E, R, D, n, 0, margin=1.0, params=c["params"])
        assert L.kge_transe_relation_copies(ctypes.byref(con._desc), B) == want_copies
        con.forward_counts(device_batch(c["batch"]), B, B, B * n)
        got = con._counts.cpu().numpy().astype(np.int64)
        loss = float(con._loss.item())
        con._counts.zero_()
    finally:
        L.kge_set_option(b"counts_force_sort", 0)
        L.kge_set_option(b"counts_krel", 4)
    bad_rows = np.nonzero((got != c["want"]).any(1))[0]
    parity_report("size_gate_exact_counts[E=%d R=%d D=%d n=%d B=%d krel=%d sort=%d]" % (E, R, D, n, B, krel, sort),
                  rows_differing=len(bad_rows), largest_count_difference=int(np.abs(got - c["want"]).max()),
                  relation_rows_differing=int((bad_rows >= E).sum()), bound_rows=EXACT_COUNT_ROWS_BOUND)
    assert len(bad_rows) <= EXACT_COUNT_ROWS_BOUND, (len(bad_rows), bad_rows[:10], np.abs(got - c["want"]).max())
    if with_loss:
        assert abs(loss - c["loss"]) <= RTOL * abs(c["loss"]), (loss, c["loss"])


def case_id(case):
    return "-".join(str(x) for x in case)


# ---- C1: relation-row copies -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,sort", [(c, s) for c in sg.EXACT_CASES for s in (0, 1)], ids=lambda v: case_id(v) if isinstance(v, tuple) else "sort%d" % v)
def test_relation_copies_exact_count_image(case, sort):
    """B = 4096: copy b & 3 of the relation rows (4 * R <= 2 (E + R)), 2 copies at E = 10, R = 40 (the halving rule), option
    counts_krel = 2 / 8 / 64 at E = 2000; B = 4095: no copies; B = 4097: group 4096 returns to copy 0.  Widths 16 / 64 / 100 /
    200 take the team shapes 16x4 / 32x4 / 64x4 with natural-layout records, 7 and 50 the scalar emit kernel whose records
    segsum_kernel sums as flush_run<..., NAT = false>; both reducers (bucket sort, radix sort)."""
    exact_count_image(case, sort)


@pytest.mark.parametrize("n,nr,foreign,D", sg.RELNEG_CASES)
@pytest.mark.parametrize("fused", [True, False])
def test_relation_copies_with_relation_and_foreign_negatives(n, nr, foreign, D, fused):
    """Relation negatives send records to OTHER relations' rows of the group's copy (csrc/models.hip emit kernels); foreign
    negatives defer their group to the fp32 residual pass.  The form of test_transe_sign_count_gradient_matches_oracle: an SGD
    step with lr = 1 read back as a gradient, through the fused step (segapply_kernel) and the two-call step (segsum_kernel)."""
    E, R, B = sg.RELNEG_E, sg.RELNEG_R, sg.RELNEG_B
    c = sg.relneg_case(n, nr, foreign, D)
    params, g_o, loss_o = c["params"], c["grads"], c["loss"]
    bh, bt, br = c["batch"]
    con = make_engine("transe", E, R, D, n, nr, margin=sg.RELNEG_MARGIN, opt="SGD", alpha=1.0, params=params)
    con.fused_counts = fused
    assert con.use_counts and lib().kge_transe_relation_copies(ctypes.byref(con._desc), B) == 4
    loss_g = con.train_step(bh, bt, br, None)
    assert abs(loss_g - loss_o) <= RTOL * abs(loss_o)
    got = con.get_parameters()
    unit = 1.0 / (B * (n + nr))
    flips = {}
    for k in g_o:
        g_g = params[k].astype(np.float64) - got[k].astype(np.float64)
        quantum = np.abs(params[k]).max() * 2.0 ** -23          # p - 1.0 * g is rounded to fp32 at the parameter's magnitude
        diff = np.abs(g_g - g_o[k])
        bad_rows = np.nonzero((diff > RTOL * np.abs(g_o[k]).max() + quantum).any(1))[0]
        min_norm = np.sqrt((params[k].astype(np.float64) ** 2).sum(1)).min()
        flips[k] = len(bad_rows)
        assert len(bad_rows) <= SIGN_FLIP_ROWS_BOUND, (k, len(bad_rows))
        assert diff.max() <= 2.05 * unit / min_norm + RTOL * np.abs(g_o[k]).max() + quantum, (k, diff.max())
    parity_report("size_gate_relneg[D=%d n=%d nr=%d foreign=%.1f fused=%d]" % (D, n, nr, foreign, fused),
                  rows_with_a_sign_flip=flips, bound_rows=SIGN_FLIP_ROWS_BOUND)
    assert not con._counts.any().item()
    for g in con.get_gradients().values():
        assert not g.any()


@pytest.mark.parametrize("dim", [16, 100])
@pytest.mark.parametrize("opt", ["SGD", "Adam"])
@pytest.mark.parametrize("cap", [0, 7])
def test_fused_step_equals_the_two_call_step_with_relation_copies(dim, opt, cap):
    """test_fused_step_equals_the_two_call_step_on_sampled_batches on a graph whose batches have 4500 groups: six device-sampled
    steps, bit for bit; the first step's loss also against the oracle's on the same batch."""
    E, R, h, t, r = sg.fused_graph()
    arrays, n = (E, R, h, t, r), sg.FUSED_NEG
    a = engine(None, dim, sg.FUSED_NBATCHES, n, opt, fused=True, cap=cap, arrays=arrays)
    B = a.batch_size
    assert B >= 4096 and a.lib.kge_transe_relation_copies(ctypes.byref(a._desc), B) == 4
    s0 = a.get_stream_states()
    dev, n_pos = a.sample_device()                                   # the batch the first step will draw ...
    first = dev.cpu().numpy().astype(np.int64)
    a.lib.kge_set_stream_states(s0.ctypes.data, 8)                   # ... from the same rng states
    assert n_pos == B
    loss_o, _ = oracle.Model("transe", E, R, dim, dim, margin=1.0, params=a.get_parameters()).grad(first[0], first[1], first[2], B, n)
    losses_a = [a.train_step() for _ in range(6)]
    sa = state(a)
    a.lib.kge_set_option(b"counts_fused_cap", 0)
    b = engine(None, dim, sg.FUSED_NBATCHES, n, opt, fused=False, arrays=arrays, streams=s0)
    losses_b = [b.train_step() for _ in range(6)]
    sb = state(b)
    assert abs(losses_a[0] - loss_o) <= RTOL * abs(loss_o), (losses_a[0], loss_o)
    assert losses_a == losses_b
    for k in sb:
        assert np.array_equal(sa[k], sb[k]), (k, float(np.abs(sa[k].astype(np.float64) - sb[k]).max()))
    assert not sa["counts"].any()
    assert a.get_stream_states().tolist() == b.get_stream_states().tolist()


# ---- C2: chunk lengths of the float-record segmented sum ------------------------------------------------------------------------

@pytest.mark.parametrize("model,D,B,chunk", sg.CHUNK_CASES)
def test_float_record_chunk_lengths_match_oracle(model, D, B, chunk):
    """segsum_f32_kernel at 16 (control: 2^18 - 16 records), 32 (2^18 + 16) and 64 (2^20 + 16) records per team: E = 3000, R = 5,
    so the five relations' hub copies give runs of ~64 records that straddle chunks and the entity rows many short runs.  Loss
    and every gradient table against the oracle; twice, the second time into re-zeroed accumulators."""
    import torch
    n = sg.CHUNK_NEG[model]
    c = sg.chunk_case(model, D, B)
    L = lib()
    assert L.kge_float_records_chunk_len(B * sg.RECORD_SLOTS[model](n)) == chunk
    L.kge_set_option(b"pair_counts", 0)
    try:
        con = make_engine(model, sg.CHUNK_E, sg.CHUNK_R, D, n, 0, margin=sg.CHUNK_MARGIN, params=c["params"], use_counts=False)
        assert not con.use_counts
        dev = device_batch(c["batch"])
        for _ in range(2):
            for g in con._grads:
                g.zero_()
            con.forward_backward(dev, B, B, B * n)
            torch.cuda.synchronize()
            loss_g = float(con._loss.item())
            assert abs(loss_g - c["loss"]) <= RTOL * abs(c["loss"]), (loss_g, c["loss"])
            check_gradients_with_kinks(model, c["params"], *c["batch"], B, n, D, 0, c["orc"], con.get_gradients(), c["grads"])
    finally:
        L.kge_set_option(b"pair_counts", 1)


# ---- C3: the second trip of the grid-capped kernels --------------------------------------------------------------------------------

@pytest.mark.parametrize("model,D", sg.PAIR_TRIP_CASES)
def test_pair_emit_second_trip_matches_oracle(model, D):
    """pair_emit_kernel (always 16-lane teams; csrc/pairs.hip pair_emit_blocks caps its grid at kMaxLossBlocks = 4096 workgroups
    of 256 / 16 teams = 65 536 groups): at n_pos = 65 573 the teams of workgroups 0-2 take a second group, reusing their
    lane-private LDS (hinge_const, add_stage).  D = 8 and 68 are one and two float4 per lane (Q = 1, 2).  2 % foreign negatives:
    among the second-trip groups one is deferred and one has no active hinge, the kernel's two `continue` exits."""
    import torch
    from openkeonspark_amd import _lib
    B = sg.SECOND_TRIP_B
    assert B > sg.MAX_LOSS_BLOCKS * 256 // 16
    c = sg.trip_case(model, D, 0.02)
    L = lib()
    L.kge_set_option(b"pair_counts_min_neg", 1)
    L.kge_set_option(b"float_records_min", 0)
    try:
        con = make_engine(model, sg.TRIP_E, sg.TRIP_R, D, 1, 0, margin=sg.TRIP_MARGIN, params=c["params"])
        assert L.kge_pair_path_active(ctypes.byref(con._desc), B, 1) == 1
        con.forward_backward(device_batch(c["batch"]), B, B, B)
        torch.cuda.synchronize()
        loss_g = float(con._loss.item())
        g_g = con.get_gradients()
    finally:
        L.kge_set_option(b"pair_counts_min_neg", 0)
        L.kge_set_option(b"float_records_min", 1 << 16)
    assert abs(loss_g - c["loss"]) <= RTOL * abs(c["loss"]), (loss_g, c["loss"])
    check_gradients_with_kinks(model, c["params"], *c["batch"], B, 1, D, 0, c["orc"], g_g, c["grads"])


def test_atomic_path_second_trip_matches_oracle():
    """fwdbwd_kernel at D = 16 (16-lane teams; csrc/models.hip launch_fb caps the grid at kMaxLossBlocks = 4096 workgroups of
    256 / 16 teams = 65 536 groups), memory-side atomics (float_records = 0): TransH at n_pos = 65 573."""
    import torch
    model, D, B = "transh", 16, sg.SECOND_TRIP_B
    assert B > sg.MAX_LOSS_BLOCKS * 256 // 16
    c = sg.trip_case(model, D, 0.0)
    L = lib()
    L.kge_set_option(b"float_records", 0)
    L.kge_set_option(b"pair_counts", 0)
    try:
        con = make_engine(model, sg.TRIP_E, sg.TRIP_R, D, 1, 0, margin=sg.TRIP_MARGIN, params=c["params"])
        con.forward_backward(device_batch(c["batch"]), B, B, B)
        torch.cuda.synchronize()
        loss_g = float(con._loss.item())
        g_g = con.get_gradients()
    finally:
        L.kge_set_option(b"float_records", 1)
        L.kge_set_option(b"pair_counts", 1)
    assert abs(loss_g - c["loss"]) <= RTOL * abs(c["loss"]), (loss_g, c["loss"])
    check_gradients_with_kinks(model, c["params"], *c["batch"], B, 1, D, 0, c["orc"], g_g, c["grads"])


@pytest.mark.parametrize("case,sort", [(c, s) for c in sg.EXACT_SECOND_TRIP for s in (0, 1)], ids=lambda v: case_id(v) if isinstance(v, tuple) else "sort%d" % v)
def test_transe_emit_second_trip_exact_count_image(case, sort):
    """The TransE emit kernels at D = 16 and 64 (team shape 16x4; launch_emit caps the grid at kMaxLossBlocks = 4096 workgroups of
    256 / 16 teams = 65 536 groups) at n_pos = 65 573: exact count image (with relation copies) and the loss."""
    assert case[2] <= 64 and case[4] > sg.MAX_LOSS_BLOCKS * 256 // 16
    exact_count_image(case, sort, with_loss=True)
