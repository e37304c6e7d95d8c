"""The TransE row appliers on a gradient that is known EXACTLY and independently of the device: the rows and counts are those of
the reference records of tests/dyadic_cases.batch_case(D, 25), a dozen of its rows left out as rows nothing reached -- on them
every value of g = unit inv (s - <x^, s> x^) and of y = x - lr g is a float32 value (premises, asserted on the CPU) -- plus the
all +0.0 row, the all -0.0 row and the clipped TINY row (hand-made counts where the batch did not touch them), plus a row listed
with all-zero counts, plus valid row ids with non-zero counts behind n_rows that must not be read.

  SGD        kge_transe_apply_rows_sgd, kge_transe_apply_counts_tables (adam = 0, the dense count image) and
             kge_transe_reduce_apply_records_sgd (from the reference's records; widths that are multiples of 4): EVERY element of
             both tables has the bits of the fp64 y.  Unlisted rows, the zero-count row and zero-gradient elements keep their bits,
             -0.0 included.
  bf16 SGD   kge_transe_apply_rows_sgd_bf16: the device's y is the exact one, so every moved element equals the pick of the
             restated hash (tests/bf16_ref.round_rows) -- no band, nothing left out.
  Adagrad    kge_transe_apply_rows_adagrad: accumulators a + g g bit for bit on the exact g, p by tests/test_gpu_adagrad.py's
             helpers.  kge_transe_apply_rows_adam_lazy on zero moments with beta1 = 0: m IS g, bit for bit; v = (g g)(1 - beta2)
             bit for bit; p by tests/test_gpu_lazy_rows.p_allowance.  kge_transe_apply_rows_rowadagrad and _rowadagrad_bf16: the
             row's sum of g^2 is taken in the device's own order and 64 squares of 2^-20-grained values do not fit 24 bits, so
             accumulator and p go through tests/test_gpu_row_adagrad.py's derived allowances (a_allowance, p_allowance),
             unchanged, on the exact g; a bf16 value must lie between the bf16 neighbours of the two ends of p's allowance.

The clipped rows (sum of squares below 1e-12: d = 0, inv = 1 / sqrt(1e-12f)) have g = fl(fl(unit inv) s).  HIP's default fp32
division and square root are correctly rounded and the build sets no fast-math flag, so inv = 1e6 exactly -- in fp32 numpy and in
fp64 alike (tests/test_dyadic_host.py) -- and g, a product of a power of two, 1e6 and a small integer, is exact: equality is
asserted for them like for every other row.  The TINY row's y = 2^-24 - lr g is the one value that is not a float32 value; it is
rounded once from the exact difference, on the device and in the reference."""
import ctypes
import functools

import numpy as np
import pytest

import bf16_ref
import dyadic_cases as dc

pytestmark = pytest.mark.gpu

N_NEG = 25
PAD = 5
F32 = np.float32
SPECIAL = (dc.ZERO_POS, dc.ZERO_NEG, dc.TINY)


@functools.lru_cache(maxsize=None)
def inputs(D):
    """-> dict(case, rows [n + PAD] int32 ascending then padding, counts [n + PAD, D] int32, n, full [(E + R), D] float32, g [n, D]
    float32 exact, zero_count_row, emit_rows: the rows the batch itself touched)."""
    c = dc.batch_case(D, N_NEG)
    emit_rows, emit_counts = dc.touched(c)
    rng = np.random.default_rng(40 + D)
    dropped = rng.choice(np.setdiff1d(emit_rows[emit_rows < dc.E], np.arange(10)), 12, replace=False)      # 25 negatives touch every entity:
    keep = ~np.isin(emit_rows, dropped)                                         # a dozen stay out of the list, as rows nothing reached
    rows, counts = list(emit_rows[keep]), list(emit_counts[keep])
    for ident in SPECIAL:
        if ident not in emit_rows:
            s = rng.integers(-20, 21, D)
            s[rng.random(D) < 0.3] = 0
            s[0], s[D - 1] = 7, -3
            rows.append(ident); counts.append(s)
    unlisted = np.setdiff1d(np.arange(dc.E + dc.R), rows)
    zero_count_row = int(unlisted[unlisted >= 10][0])
    rows.append(zero_count_row); counts.append(np.zeros(D, np.int64))
    order = np.argsort(rows)
    rows, counts = np.asarray(rows)[order], np.asarray(counts)[order]
    n = len(rows)
    pad_rows = unlisted[unlisted != zero_count_row][-PAD:]
    full = np.concatenate([c["ent"], c["rel"]])
    x = full[rows]
    g32 = dc.count_grad_fp32(x, counts, dc.DENOM)
    g64 = bf16_ref.gradient(x, counts, dc.DENOM)
    assert np.array_equal(g32.astype(np.float64), g64)                          # the exact gradient, the clipped rows included
    clipped = np.isin(rows, SPECIAL)
    assert np.array_equal(g32[clipped], (F32(1e6 / dc.DENOM) * counts[clipped].astype(F32)).astype(F32)) and g32[clipped].any(axis=1).all()
    return dict(case=c, n=n, full=full, g=g32, zero_count_row=zero_count_row, emit_rows=emit_rows, emit_counts=emit_counts,
                rows=np.concatenate([rows, pad_rows]).astype(np.int32),
                counts=np.concatenate([counts, np.full((PAD, D), 9)]).astype(np.int32))


def sgd_want(full, rows, counts, lr):
    """The tables after SGD on the listed rows: float32 [(E + R), D]."""
    y, g, y64, _ = dc.sgd_reference(full[rows], counts, dc.DENOM, lr)
    not_tiny = rows != dc.TINY
    assert np.array_equal(y[not_tiny].astype(np.float64), np.where(g[not_tiny] == 0, full[rows][not_tiny], y64[not_tiny]))      # exact
    want = full.copy()
    want[rows] = y
    return want


def same_bits(got, want, what):
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def env(D):
    import torch
    from openkeonspark_amd import _lib
    return torch, _lib, _lib.lib(), _lib.ModelDesc(0, 0, dc.E, dc.R, D, D, 1.0, 0)


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def tables(full):
    return dev(full[:dc.E]), dev(full[dc.E:])


def back(ent, rel):
    import torch
    torch.cuda.synchronize()
    return np.concatenate([ent.cpu().numpy(), rel.cpu().numpy()])


@pytest.mark.parametrize("lr", dc.LRS)
@pytest.mark.parametrize("D", dc.FP32_DIMS)
def test_sgd_on_listed_rows_the_dense_image_and_records(D, lr):
    torch, _lib, L, desc = env(D)
    inp = inputs(D)
    n, full, rows, counts = inp["n"], inp["full"], inp["rows"], inp["counts"]
    want = sgd_want(full, rows[:n], counts[:n], lr)
    moved = want.view(np.uint32) != full.view(np.uint32)
    assert moved[list(SPECIAL)].any(axis=1).all() and not moved[inp["zero_count_row"]].any() and not moved[rows[n:]].any()
    kept_minus_zero = (~moved) & (full == 0) & np.signbit(full)
    assert kept_minus_zero[rows[:n]].any()                                      # -0.0 elements with zero gradient inside moving rows
    d_rows, d_counts, d_n = dev(rows), dev(counts), dev(np.array([n], np.int32))
    # a. the listed rows
    ent, rel = tables(full)
    _lib.check(L.kge_transe_apply_rows_sgd(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(),
                                           d_n.data_ptr(), n + PAD, dc.DENOM, lr, None), L)
    same_bits(back(ent, rel), want, "kge_transe_apply_rows_sgd")
    # b. the dense count image
    image = np.zeros((dc.E + dc.R, D), np.int32)
    image[rows[:n]] = counts[:n]
    ent, rel = tables(full)
    d_image = dev(image)
    resid = [torch.zeros((dc.E, D), device="cuda"), torch.zeros((dc.R, D), device="cuda")]
    _lib.check(L.kge_transe_apply_counts_tables(ctypes.byref(desc), _lib.table_ptrs([ent.data_ptr(), rel.data_ptr()]), None, None,
                                                d_image.data_ptr(), _lib.table_ptrs([t.data_ptr() for t in resid]), dc.DENOM, 0, lr, 0.9,
                                                0.999, 1e-8, None), L)
    same_bits(back(ent, rel), want, "kge_transe_apply_counts_tables")
    assert not d_image.any().item()                                             # the image is re-zeroed
    # c. reduce + apply from the reference's records: the rows the batch touched
    if D % 4 == 0:
        c = inp["case"]
        w = c["want"]
        dw = int(L.kge_transe_record_dwords(ctypes.byref(desc)))
        M = len(w["keys"])
        rec = np.zeros((M, 4 * dw), np.int8)
        rec[:, :D] = w["rec"]
        d_rec, d_dst = dev(rec.view(np.int32)), dev(w["keys"].astype(np.int32))
        out_rows = torch.full((M,), -9, dtype=torch.int32, device="cuda")
        out_counts = torch.zeros((M, D), dtype=torch.int32, device="cuda")
        out_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        ent, rel = tables(full)
        _lib.check(L.kge_transe_reduce_apply_records_sgd(ctypes.byref(desc), d_rec.data_ptr(), d_dst.data_ptr(), M, ent.data_ptr(),
                                                         rel.data_ptr(), out_rows.data_ptr(), out_counts.data_ptr(), out_n.data_ptr(), dc.DENOM,
                                                         lr, None), L)
        want_c = sgd_want(full, inp["emit_rows"], inp["emit_counts"], lr)
        same_bits(back(ent, rel), want_c, "kge_transe_reduce_apply_records_sgd")
        assert int(out_n.item()) == len(inp["emit_rows"])


@pytest.mark.parametrize("lr", dc.LRS)
@pytest.mark.parametrize("D,seed,step", [(8, 0, 0), (16, 5, 3), (72, 9, 2), (200, 0xFEEDFACE12345678, 0), (264, 5, 1000), (512, 9, 2), (1024, 1, 1)])
def test_sgd_bf16_picks_what_the_hash_picks(D, seed, step, lr):
    assert D in dc.BF16_DIMS
    torch, _lib, L, desc = env(D)
    inp = inputs(D)
    n, full, rows, counts = inp["n"], inp["full"], inp["rows"], inp["counts"]
    want = sgd_want(full, rows[:n], counts[:n], lr)
    stored = bf16_ref.to_bf16(full)
    want_bits = stored.copy()
    picked = bf16_ref.round_rows(want[rows[:n]], rows[:n], seed, step)
    moved = want[rows[:n]].view(np.uint32) != full[rows[:n]].view(np.uint32)
    want_bits[rows[:n]] = np.where(moved, picked, stored[rows[:n]])
    inexact = bf16_ref.widen(bf16_ref.to_bf16(want[rows[:n]])) != want[rows[:n]]
    print("moved %d elements, %d of them between two bf16 values" % (moved.sum(), (moved & inexact).sum()))
    assert (moved & inexact).sum() > 50 or D <= 16
    ent, rel = dev(stored[:dc.E].view(np.int16)), dev(stored[dc.E:].view(np.int16))
    d_rows, d_counts, d_n = dev(rows), dev(counts), dev(np.array([n], np.int32))      # (held until the launch has run)
    _lib.check(L.kge_transe_apply_rows_sgd_bf16(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(),
                                                d_n.data_ptr(), n + PAD, dc.DENOM, lr, ctypes.c_uint64(seed), ctypes.c_uint64(step), None), L)
    torch.cuda.synchronize()
    got = np.concatenate([ent.cpu().numpy(), rel.cpu().numpy()]).view(np.uint16)
    np.testing.assert_array_equal(got, want_bits)                               # every element of both tables: no band, share left out 0


@pytest.mark.parametrize("D", dc.FP32_DIMS)
def test_adagrad_and_lazy_adam_on_the_exact_gradient(D):
    from test_gpu_adagrad import A0, _check_against_rule, adagrad_rule_fp32
    from test_gpu_lazy_rows import p_allowance as adam_p_allowance
    torch, _lib, L, desc = env(D)
    inp = inputs(D)
    n, full, rows, counts = inp["n"], inp["full"], inp["rows"], inp["counts"]
    G = np.zeros_like(full)
    G[rows[:n]] = inp["g"]
    rng = np.random.default_rng(D)
    d_rows, d_counts, d_n = dev(rows), dev(counts), dev(np.array([n], np.int32))
    lr = 0.05
    # Adagrad: one accumulator per element
    A = (A0 + rng.random(full.shape)).astype(F32)
    ent, rel = tables(full)
    a_ent, a_rel = tables(A)
    _lib.check(L.kge_transe_apply_rows_adagrad(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), a_ent.data_ptr(), a_rel.data_ptr(),
                                               d_rows.data_ptr(), d_counts.data_ptr(), d_n.data_ptr(), n + PAD, dc.DENOM, lr, None), L)
    got_p, got_a = back(ent, rel), back(a_ent, a_rel)
    want_p, want_a, step = adagrad_rule_fp32(full, A, G, lr)
    _check_against_rule(got_p, got_a, want_p, want_a, step, "Adagrad, width %d" % D)
    still = G == 0
    same_bits(got_p[still], full[still], "zero-gradient elements")
    same_bits(got_a[still], A[still], "zero-gradient accumulators")
    # lazy Adam on zero moments, beta1 = 0: m is the gradient itself
    b2, eps, lr_t = 0.999, 1e-8, 0.01
    ent, rel = tables(full)
    zeros = [torch.zeros((rows_, D), device="cuda") for rows_ in (dc.E, dc.R, dc.E, dc.R)]
    _lib.check(L.kge_transe_apply_rows_adam_lazy(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), zeros[0].data_ptr(), zeros[1].data_ptr(),
                                                 zeros[2].data_ptr(), zeros[3].data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), d_n.data_ptr(),
                                                 n + PAD, dc.DENOM, lr_t, 0.0, b2, eps, None, None), L)
    got_p, got_m, got_v = back(ent, rel), back(zeros[0], zeros[1]), back(zeros[2], zeros[3])
    same_bits(got_m, G + F32(0), "m = g")                                       # (+ 0: the kernels form g + 0.0f, no -0.0)
    want_v = ((G * G).astype(F32) * (F32(1) - F32(b2))).astype(F32)
    same_bits(got_v, want_v, "v = g g (1 - beta2)")
    with np.errstate(invalid="ignore", divide="ignore"):
        step = np.where(G != 0, ((F32(lr_t) * G) / (np.sqrt(want_v) + F32(eps))).astype(F32), F32(0))
    want_p = (full - step).astype(F32)
    off = np.abs(got_p.astype(np.float64) - want_p)
    slack = np.where(step != 0, adam_p_allowance(want_p, step), 0.0)
    assert (off <= slack).all(), float((off - slack).max())
    same_bits(got_p[still], full[still], "zero-gradient elements under lazy Adam")


@pytest.mark.parametrize("D", sorted(set(dc.FP32_DIMS) | set(dc.BF16_DIMS)))
def test_row_adagrad_on_the_exact_gradient(D):
    from test_gpu_adagrad import A0
    from test_gpu_row_adagrad import a_allowance, p_allowance, row_rule_fp64
    torch, _lib, L, desc = env(D)
    inp = inputs(D)
    n, full, rows, counts = inp["n"], inp["full"], inp["rows"], inp["counts"]
    G = np.zeros_like(full)
    G[rows[:n]] = inp["g"]
    rng = np.random.default_rng(D + 1)
    A = (A0 + rng.random(dc.E + dc.R)).astype(F32)
    d_rows, d_counts, d_n = dev(rows), dev(counts), dev(np.array([n], np.int32))
    lr = 0.05
    bare = ~(G != 0).any(axis=1)
    assert bare[inp["zero_count_row"]] and bare[rows[n:]].all() and not bare[list(SPECIAL)].any()
    if D in dc.FP32_DIMS:
        ent, rel = tables(full)
        a_ent, a_rel = dev(A[:dc.E]), dev(A[dc.E:])
        _lib.check(L.kge_transe_apply_rows_rowadagrad(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), a_ent.data_ptr(), a_rel.data_ptr(),
                                                      d_rows.data_ptr(), d_counts.data_ptr(), d_n.data_ptr(), n + PAD, dc.DENOM, lr, None), L)
        got_p, got_a = back(ent, rel), back(a_ent, a_rel)
        want_p, want_a, inc, step = row_rule_fp64(full, A, G, lr)
        da = a_allowance(want_a, inc, D)
        assert (np.abs(got_a.astype(np.float64) - want_a) <= da).all()
        assert (np.abs(got_p.astype(np.float64) - want_p) <= p_allowance(full.astype(np.float64), want_p, step, want_a, da)).all()
        same_bits(got_p[G == 0], full[G == 0], "zero-gradient elements")
        same_bits(got_a[bare], A[bare], "accumulators of the rows without gradient")
        # (a few rows' whole increment q / D is below the accumulator's ulp: the others must grow)
        grew = inc > np.spacing(A).astype(np.float64)
        assert (got_a[grew] > A[grew]).all() and (got_a >= A).all() and grew.sum() > 400
    if D in dc.BF16_DIMS:
        stored = bf16_ref.to_bf16(full)
        ent, rel = dev(stored[:dc.E].view(np.int16)), dev(stored[dc.E:].view(np.int16))
        a_ent, a_rel = dev(A[:dc.E]), dev(A[dc.E:])
        _lib.check(L.kge_transe_apply_rows_rowadagrad_bf16(ctypes.byref(desc), ent.data_ptr(), rel.data_ptr(), a_ent.data_ptr(), a_rel.data_ptr(),
                                                           d_rows.data_ptr(), d_counts.data_ptr(), d_n.data_ptr(), n + PAD, dc.DENOM, lr,
                                                           ctypes.c_uint64(7), ctypes.c_uint64(3), None), L)
        torch.cuda.synchronize()
        got = np.concatenate([ent.cpu().numpy(), rel.cpu().numpy()]).view(np.uint16)
        got_a = back(a_ent, a_rel)
        want_p, want_a, inc, step = row_rule_fp64(full, A, G, lr)
        assert (np.abs(got_a.astype(np.float64) - want_a) <= a_allowance(want_a, inc, D)).all()
        same_bits(got_a[bare], A[bare], "accumulators of the rows without gradient")
        still = G == 0
        np.testing.assert_array_equal(got[still], stored[still])                # zero gradient: the stored bits stay, -0.0 included
        # a moved element lies between the bf16 neighbours of the two ends of the fp32 allowance around the rule's p
        slack = p_allowance(full.astype(np.float64), want_p, step, want_a, a_allowance(want_a, inc, D))
        ends = [bf16_ref.widen(b).astype(np.float64) for y in (want_p - slack, want_p + slack) for b in bf16_ref.neighbours(y)]
        v = bf16_ref.widen(got).astype(np.float64)
        assert ((v >= np.minimum.reduce(ends)) & (v <= np.maximum.reduce(ends)))[~still].all()
