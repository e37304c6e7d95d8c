"""ONE call of kge_transe_train_step_counts (sampler_shaped = 1, SGD) on the exact tables and batches of tests/dyadic_cases.py,
against the fp64 definition bit for bit: emit (tests/bf16_ref.emit), per-row counts, g = unit inv (s - <x^, s> x^) and
y = x - lr g are all float32 values there (premises, asserted on the CPU), so both tables must hold the fp64 y in EVERY bit,
the loss must have the bits of the fp64 loss, the count image must be all zero on return and a row no record reached must keep
its bits, -0.0 included.  denom = 2^10; lr = 1 with 25 negatives (every entity but the clipped TINY row is touched, the relation
rows by a thousand records each) and lr = 1/4 with one negative (two fifths of the rows untouched); option counts_fused_cap 0 (the
default) and 7 (nearly every row is cut into pieces and goes through the count image), restored afterwards.  One step only: after
an update the rows are no longer dyadic."""
import ctypes

import numpy as np
import pytest

import dyadic_cases as dc

pytestmark = pytest.mark.gpu

DIMS = [16, 50, 200, 520]


@pytest.mark.parametrize("cap", [0, 7])
@pytest.mark.parametrize("lr,n_neg", [(1.0, 25), (0.25, 1)])
@pytest.mark.parametrize("D", DIMS)
def test_one_fused_step_equals_the_definition_bit_for_bit(D, lr, n_neg, cap):
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    c = dc.batch_case(D, n_neg)
    want = c["want"]
    assert want["deferred"] == 0
    rows, counts = dc.touched(c)
    full = np.concatenate([c["ent"], c["rel"]])
    y, g, y64, _ = dc.sgd_reference(full[rows], counts, dc.DENOM, lr)
    assert np.array_equal(y.astype(np.float64), np.where(g == 0, full[rows], y64)) and dc.TINY not in rows      # exact
    want_full = full.copy()
    want_full[rows] = y
    untouched = np.setdiff1d(np.arange(dc.E + dc.R), rows)
    assert dc.TINY in untouched and (n_neg > 1 or len(untouched) > 50)
    desc = _lib.ModelDesc(0, 0, dc.E, dc.R, D, D, c["margin"], 0)
    assert L.kge_transe_counts_supported(ctypes.byref(desc), n_neg) == 1
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ent, rel = d(c["ent"]), d(c["rel"])
    bh, bt, br = d(c["bh"]), d(c["bt"]), d(c["br"])
    image = torch.zeros((dc.E + dc.R, D), dtype=torch.int32, device="cuda")
    resid = [torch.zeros((dc.E, D), device="cuda"), torch.zeros((dc.R, D), device="cuda")]
    loss = torch.full((1,), -1.0, device="cuda")
    L.kge_set_option(b"counts_fused_cap", cap)
    try:
        L.kge_set_option(b"tables_changed", 1)      # fresh tensors may reuse an address whose 1/|row| table the engine still holds
        _lib.check(L.kge_transe_train_step_counts(ctypes.byref(desc), _lib.table_ptrs([ent.data_ptr(), rel.data_ptr()]), None, None,
                                                  bh.data_ptr(), bt.data_ptr(), br.data_ptr(), dc.N_POS, n_neg, dc.STRIDE, dc.DENOM,
                                                  image.data_ptr(), _lib.table_ptrs([t.data_ptr() for t in resid]), 1, 0, lr, 0.9, 0.999,
                                                  1e-8, loss.data_ptr(), None), L)
        torch.cuda.synchronize()
    finally:
        L.kge_set_option(b"counts_fused_cap", 0)
        L.kge_set_option(b"tables_changed", 1)
    got = np.concatenate([ent.cpu().numpy(), rel.cpu().numpy()])
    got_loss = np.float32(loss.item())
    print("loss %.9g reference %.9g; %d rows touched" % (got_loss, want["loss"], len(rows)))
    assert got_loss.view(np.uint32) == np.float32(want["loss"]).view(np.uint32)
    np.testing.assert_array_equal(got[untouched].view(np.uint32), full[untouched].view(np.uint32))
    np.testing.assert_array_equal(got.view(np.uint32), want_full.view(np.uint32))
    assert not image.any().item() and not resid[0].any().item() and not resid[1].any().item()
