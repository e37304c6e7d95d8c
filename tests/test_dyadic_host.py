"""The premises of tests/dyadic_cases.py for every case the device tests use (tests/test_gpu_dyadic_emit.py, _rows.py, _step.py),
on the references alone: a fixture that is not exact, has no tie, no one-quantum miss, no exact zero of each kind or no 63 / 64
boundary fails HERE, on a machine without a GPU.  The builders themselves raise when no margin meets the premises; the tests
below restate the figures that matter and print them."""
import numpy as np
import pytest

import bf16_ref
import dyadic_cases as dc

BATCH_DIMS = sorted(set(dc.FP32_DIMS) | set(dc.BF16_DIMS) | {520})
LIST_DIMS = sorted(set(dc.FP32_DIMS) | set(dc.SHARED_BF16_DIMS))


def check_stats(c):
    s = c["stats"]
    total, zeros, both, cancel, minus = s["zeros"]
    print("D %d margin %g: %d ties, %d one quantum above, %d below; %d of %d pairs active; %.0f %% of e exact zeros (%d all-zero operands, "
          "%d cancellations, %d with a -0.0 operand)" % (c["D"], c["margin"], s["ties"], s["above"], s["below"], s["active"], s["pairs"],
                                                         100.0 * zeros / total, both, cancel, minus))
    assert min(s["ties"], s["above"], s["below"]) >= 20 and zeros >= 0.05 * total and min(both, cancel, minus) > 0
    assert 0 < s["active"] < s["pairs"]


@pytest.mark.parametrize("D", BATCH_DIMS)
def test_batches_meet_the_premises(D):
    negs = dc.NEGS + ([dc.BOUNDARY_NEG] if D % 8 == 0 else [])
    for n_neg in negs:
        c = dc.batch_case(D, n_neg)
        dc.premises(c)                                      # (again, on the cached case: nothing in it has changed)
        check_stats(c)
        want = c["want"]
        if n_neg >= 63:
            assert want["active"][dc.X_POS] == 63
        if n_neg == dc.BOUNDARY_NEG:
            assert want["deferred"] >= 1 and (want["keys"].reshape(-1, dc.N_POS)[:, dc.Y_POS] == -1).all()


@pytest.mark.parametrize("D", LIST_DIMS)
def test_lists_meet_the_premises(D):
    for P, N in dc.SHARED_SHAPES:
        for c in (dc.lists_case(D, P, N), dc.chunks_case(D, P, N)):
            dc.premises(c)
            check_stats(c)
            assert (c["pair"][c["masked_positive"]] & 2).all()
            if N >= 8:
                assert (c["cand"] >= dc.E).any() and (c["cand"] < 0).any()


@pytest.mark.parametrize("D", [8, 50, 200, 1024])
def test_tables_are_what_the_module_says(D):
    ent, rel = dc.dyadic_tables(dc.E, dc.R, D, 5)
    for tab, special in ((ent, (dc.ZERO_POS, dc.ZERO_NEG, dc.TINY)), (rel, (dc.ZERO_REL,))):
        rows = np.setdiff1d(np.arange(len(tab)), special)
        x = tab[rows].astype(np.float64)
        nz = x != 0
        s = nz.sum(1)
        assert np.isin(s, (1, 4, 16, 64)).all() and (s <= D // 2).all()
        mag = np.abs(x).max(1)
        assert (np.abs(x)[nz] == np.repeat(mag, s)).all() and np.isin(mag, (0.25, 0.5, 1.0, 2.0)).all()
        norm = np.sqrt((x * x).sum(1))
        assert (np.log2(norm) == np.round(np.log2(norm))).all()                  # the norm is a power of two
        assert (np.signbit(tab[rows]) & ~nz).any() and (~np.signbit(tab[rows]) & ~nz).any()      # both zeros
        win = min(D, 24)
        assert nz[:, :win].any() and nz[:, D - win:].any() and (tab is rel or (nz[:, 0].any() and nz[:, D - 1].any()))
    assert np.array_equal(bf16_ref.widen(bf16_ref.to_bf16(ent)).view(np.uint32), ent.view(np.uint32))
    assert np.count_nonzero(ent[dc.TINY]) == 4 and (ent[dc.TINY].astype(np.float64) ** 2).sum() == 2.0 ** -46


def test_the_clipped_rows_have_one_gradient_in_fp32_and_fp64():
    """inv = 1 / sqrt(1e-12) is 1e6 in both, d = 0: g = unit * 1e6 * s, exact in fp32 for |s| <= 127 at unit = 2^-10."""
    assert float(np.float32(1) / np.sqrt(np.float32(1e-12))) == 1e6 == 1.0 / np.sqrt(1e-12)
    ent, _ = dc.dyadic_tables(dc.E, dc.R, 16, 5)
    x = ent[[dc.ZERO_POS, dc.ZERO_NEG, dc.TINY]]
    counts = np.arange(-24, 24).reshape(3, 16) * 5
    g32 = dc.count_grad_fp32(x, counts, dc.DENOM)
    assert np.array_equal(g32.astype(np.float64), bf16_ref.gradient(x, counts, dc.DENOM))
    assert np.array_equal(g32, (np.float32(2.0 ** -10 * 1e6) * counts.astype(np.float32)).astype(np.float32))
