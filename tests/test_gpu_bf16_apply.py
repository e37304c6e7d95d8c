"""kge_transe_apply_rows_sgd_bf16 / kge_transe_apply_rows_rowadagrad_bf16 alone, on hand-made row lists and counts: entity rows,
a relation row, a row listed with all-zero counts, elements with zero count inside a touched row (they move: the normalisation's
backward gives them a gradient) and elements with zero count AND zero value (gradient exactly zero: their bits stay).

Against the fp64 rule y_ref (tests/bf16_ref.py) on the widened rows:
  * every stored value is one of the two bf16 neighbours of y_ref;
  * it equals the pick of the restated hash wherever that pick is decided by more than 4 fp32 ulps of y, i.e. frac * 65536 + rnd
    is not within 4 of a multiple of 65536 (frac: where y_ref lies between its neighbours; the device forms y in fp32, a few ulps
    from y_ref).  The share of elements that band leaves out is computed from the reference alone BEFORE the comparison and must
    be at most 1e-3 (a band of 9 in 65536 around each of two multiples: about 1.2e-4 .. 2.7e-4 for spread-out low bits);
  * rows that are not listed, rows listed with zero counts, their accumulators and zero-gradient elements keep their bits;
  * row-wise Adagrad's accumulators are within 1e-6 relative of fp64.
lr = 0.5 moves an element by about a percent of its value: thousands of fp32 ulps, several bf16 ulps.

The sub-ulp case: every update is 1/16 of a bf16 ulp (4096 elements, 16 steps); the summed movement must be within 4 standard
deviations of the exact one, where round-to-nearest would not move at all."""
import ctypes

import numpy as np
import pytest

import bf16_ref as ref

pytestmark = pytest.mark.gpu

E, R = 500, 7
TRANSE = 0
DENOM = 301 * 5
BAND = 4


def apply_rows(kind, D, ent, rel, acc, rows, counts, lr, seed, step, denom=DENOM, pad=5):
    """One call on copies of the tables (uint16 bits) and accumulators -> (ent, rel, acc_ent, acc_rel) afterwards."""
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    desc = _lib.ModelDesc(TRANSE, 0, E, R, D, D, 1.0, 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_ent, t_rel = d(ent.view(np.int16)), d(rel.view(np.int16))
    n = len(rows)
    d_rows = d(np.concatenate([rows, np.full(pad, 1, np.int32)]).astype(np.int32))      # entries past n_rows are not read
    d_counts = d(np.concatenate([counts, np.full((pad, D), 9, np.int32)]).astype(np.int32))
    d_n = d(np.array([n], np.int32))
    seed, step = ctypes.c_uint64(seed), ctypes.c_uint64(step)
    if kind == "sgd":
        _lib.check(L.kge_transe_apply_rows_sgd_bf16(ctypes.byref(desc), t_ent.data_ptr(), t_rel.data_ptr(), d_rows.data_ptr(),
                                                    d_counts.data_ptr(), d_n.data_ptr(), n + pad, denom, lr, seed, step, None), L)
        a_ent = a_rel = None
    else:
        a_ent, a_rel = d(acc[0]), d(acc[1])
        _lib.check(L.kge_transe_apply_rows_rowadagrad_bf16(ctypes.byref(desc), t_ent.data_ptr(), t_rel.data_ptr(), a_ent.data_ptr(),
                                                           a_rel.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), d_n.data_ptr(), n + pad,
                                                           denom, lr, seed, step, None), L)
        a_ent, a_rel = a_ent.cpu().numpy(), a_rel.cpu().numpy()
    torch.cuda.synchronize()
    return t_ent.cpu().numpy().view(np.uint16), t_rel.cpu().numpy().view(np.uint16), a_ent, a_rel


def hand_made(D, seed):
    rng = np.random.default_rng(seed)
    ent = ref.to_bf16(rng.normal(0, 0.1, (E, D)).astype(np.float32))
    rel = ref.to_bf16(rng.normal(0, 0.1, (R, D)).astype(np.float32))
    rows = np.array([3, 17, 499, E + 2, 42, 0, 250, E + R - 1, 77], np.int32)      # 42: listed with all-zero counts
    counts = rng.integers(-20, 21, (len(rows), D)).astype(np.int32)
    counts[rng.random(counts.shape) < 0.3] = 0                                      # zero counts inside touched rows
    counts[4] = 0
    counts[6, 1:] = 0                                                               # a row touched in ONE element
    counts[6, 0] = 5
    zero_at = np.arange(0, D, 5)                                                    # zero count AND zero value: gradient exactly zero
    ent[17, zero_at] = 0; counts[1, zero_at] = 0
    ent[17, zero_at[::2]] = 0x8000                                                  # ... half of them -0.0
    acc = [(0.1 + rng.random(E)).astype(np.float32), (0.1 + rng.random(R)).astype(np.float32)]
    return ent, rel, acc, rows, counts


@pytest.mark.parametrize("kind", ["sgd", "row_adagrad"])
@pytest.mark.parametrize("D,seed,step", [(8, 0, 0), (24, 5, 3), (200, 0xFEEDFACE12345678, 0), (200, 5, 1000), (520, 9, 2), (1024, 1, 1)])
def test_listed_rows_against_the_rule(kind, D, seed, step):
    ent, rel, acc, rows, counts = hand_made(D, 100 + D)
    lr = 0.5
    live = np.array([i for i in range(len(rows)) if counts[i].any()])
    full = np.concatenate([ent, rel])
    x = ref.widen(full[rows[live]])
    a0 = np.concatenate(acc)[rows[live]] if kind == "row_adagrad" else None
    y_ref, a_ref, g = ref.update(x, counts[live], DENOM, lr, a0)
    wide = (g != 0) & (rows[live] != 250)[:, None]      # (the row touched in one element moves its other elements by less)
    assert (np.abs(y_ref - x)[wide] > 64 * np.spacing(np.abs(x[wide]))).mean() > 0.95      # updates span many fp32 ulps
    lo, hi = ref.neighbours(y_ref)
    lo_v, hi_v = np.abs(ref.widen(lo).astype(np.float64)), np.abs(ref.widen(hi).astype(np.float64))
    frac = np.where(hi_v > lo_v, (np.abs(y_ref) - lo_v) / np.where(hi_v > lo_v, hi_v - lo_v, 1.0), 0.0)
    rnd = ref.round_bits(seed, step, rows[live].reshape(-1, 1), D, np.arange(D).reshape(1, -1)).astype(np.float64)
    t = frac * 65536.0 + rnd
    near = np.abs(t - 65536.0 * np.round(t / 65536.0)) <= BAND
    moved = g != 0
    share = (near & moved).sum() / max(moved.sum(), 1)
    print("band share %.3g of %d moved elements" % (share, moved.sum()))
    assert share <= 1e-3
    pick = np.where(t >= 65536.0, hi, lo)

    got_ent, got_rel, a_ent, a_rel = apply_rows(kind, D, ent, rel, acc, rows, counts, lr, seed, step)
    got_full = np.concatenate([got_ent, got_rel])
    got = got_full[rows[live]]
    assert ((got == lo) | (got == hi)).all()
    decided = moved & ~near
    np.testing.assert_array_equal(got[decided], pick[decided])
    np.testing.assert_array_equal(got[~moved], full[rows[live]][~moved])            # zero gradient: the bits stay (-0.0 included)
    assert (~moved).sum() >= len(np.arange(0, D, 5))
    untouched = np.ones(E + R, bool)
    untouched[rows[live]] = False
    assert untouched[42] and untouched.sum() == E + R - len(live)
    np.testing.assert_array_equal(got_full[untouched], full[untouched])             # not listed, or listed with zero counts
    if kind == "row_adagrad":
        got_a, a_all = np.concatenate([a_ent, a_rel]), np.concatenate(acc)
        np.testing.assert_array_equal(got_a[untouched], a_all[untouched])
        rel_err = np.abs(got_a[rows[live]].astype(np.float64) - a_ref) / a_ref
        print("accumulators: largest relative error %.3g" % rel_err.max())
        grew = a_ref - a_all[rows[live]] > np.spacing(a_all[rows[live]])      # (a row touched in one element adds less than an ulp)
        assert (rel_err <= 1e-6).all() and (got_a[rows[live]] >= a_all[rows[live]]).all() and (got_a[rows[live]] > a_all[rows[live]])[grew].all()
        assert grew.sum() >= len(live) - 1


@pytest.mark.parametrize("kind", ["sgd", "row_adagrad"])
def test_the_same_call_gives_the_same_bits_and_other_seeds_or_steps_others(kind):
    D = 200
    ent, rel, acc, rows, counts = hand_made(D, 7)
    a = apply_rows(kind, D, ent, rel, acc, rows, counts, 0.5, 11, 4)
    b = apply_rows(kind, D, ent, rel, acc, rows, counts, 0.5, 11, 4)
    for u, v in zip(a, b):
        if u is not None:
            np.testing.assert_array_equal(u, v)
    assert (a[0] != apply_rows(kind, D, ent, rel, acc, rows, counts, 0.5, 12, 4)[0]).sum() > 50
    assert (a[0] != apply_rows(kind, D, ent, rel, acc, rows, counts, 0.5, 11, 5)[0]).sum() > 50


def test_sub_ulp_updates_move_the_rows_in_expectation():
    """8 rows of 512 elements, all 1.5; counts +1 / -1 by blocks of 64 columns, orthogonal to the row, so g = unit * inv * s with
    inv = 1 / (1.5 sqrt(512)) and lr is chosen to make |lr g| = 2^-11: 1/16 of the bf16 ulp 2^-7 at 1.5.  Each step's exact
    movement is taken from the fp64 rule on the stored rows; stochastic rounding is a martingale around it with variance
    sum p (1 - p) ulp^2.  Round-to-nearest would leave every element at 1.5."""
    D, n, steps, seed = 512, 8, 16, 2024
    ent = np.zeros((E, D), np.uint16); rel = ref.to_bf16(np.full((R, D), 0.25, np.float32))
    rows = np.arange(10, 10 + n).astype(np.int32)
    ent[:] = ref.to_bf16(np.float32(0.5))
    ent[rows] = ref.to_bf16(np.float32(1.5))
    counts = np.tile(np.where((np.arange(D) // 64) % 2 == 0, 1, -1).astype(np.int32), (n, 1))
    lr = float(np.float32(2.0 ** -11 * 1.5 * np.sqrt(512.0)))
    ulp = 2.0 ** -7
    start = ref.widen(ent[rows]).astype(np.float64)
    expected, var = 0.0, 0.0
    cur = ent
    for step in range(steps):
        x = ref.widen(cur[rows])
        y_ref, _, g = ref.update(x, counts, 1, lr)
        move = y_ref - x
        assert (np.abs(np.abs(move) / ulp - 1 / 16) < 1e-3).all()      # every update is 1/16 of a bf16 ulp
        assert (ref.to_bf16(y_ref.astype(np.float32)) == cur[rows]).all()      # round-to-nearest would not move
        p = np.abs(move) / ulp
        expected += (move * np.sign(move)).sum()
        var += (p * (1 - p) * ulp * ulp).sum()
        cur, _, _, _ = apply_rows("sgd", D, cur, rel, None, rows, counts, lr, seed, step, denom=1)
        assert (np.abs(ref.widen(cur[rows]).astype(np.float64) - x) <= ulp).all()
    toward = np.where(counts > 0, -1.0, 1.0)       # y = x - lr g: positive counts move down
    moved = ((ref.widen(cur[rows]).astype(np.float64) - start) * toward).sum()
    print("summed movement %.6g exact %.6g sd %.3g" % (moved, expected, np.sqrt(var)))
    assert n * D == 4096 and expected > 0.9 * 4096 * 16 * ulp / 16
    assert abs(moved - expected) <= 4 * np.sqrt(var)
    assert moved > 0.5 * expected


def test_bad_arguments_are_refused():
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(1 << 12, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    for D, why in ((100, "multiple of 8"), (1032, "up to 1024")):
        desc = _lib.ModelDesc(TRANSE, 0, E, R, D, D, 1.0, 0)
        with pytest.raises(_lib.KgeError) as e:
            _lib.check(L.kge_transe_apply_rows_sgd_bf16(ctypes.byref(desc), p, p, p, p, p, 1, 1, 0.1, 0, 0, None), L)
        assert why in str(e.value)
    desc = _lib.ModelDesc(TRANSE, 0, E, R, 24, 24, 1.0, 0)
    assert L.kge_transe_apply_rows_rowadagrad_bf16(ctypes.byref(desc), p, p, None, None, p, p, p, 1, 1, 0.1, 0, 0, None) != 0
    assert L.kge_transe_apply_rows_sgd_bf16(ctypes.byref(desc), p, p, p, p, p, 1, 0, 0.1, 0, 0, None) != 0
    L.kge_clear_error()
