"""opt_method "Adagrad": TF1's AdagradOptimizer on the touched-rows paths (TransE sign counts, TransE / TransH / TransD float
records) and as a dense sweep (TransR).  Per element, in fp32 (csrc/optim_dev.hpp adagrad_one):

    if (g != 0) { a = a + g*g;  p = p - (lr*g) / sqrt(a); }

no epsilon, accumulators from Config.adagrad_initial_accumulator (0.1).  An element with zero gradient keeps p and a bit for
bit, so "only the touched rows" and "every row" are the same rule -- checked here as such (test_touched_rows_equal_the_dense_sweep).

One process: each stage alone against the rule in fp32 numpy (accumulators bit for bit: sums and products only, in a fixed
order; values to the accuracy of the hardware square root), whole steps against the rule on the CPU oracle's gradient, the
errors, and reproducibility.  Ranks: tests/test_gpu_adagrad_dp.py; the driver and checkpoints: tests/test_gpu_adagrad_checkpoint.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity_report
from oracle import oracle
from test_gpu_lazy_rows import ENT_SIDE, RTOL, touched_rows
from test_gpu_models import rand_batch, seed_of

pytestmark = pytest.mark.gpu

A0 = 0.1                 # Config.adagrad_initial_accumulator's default (TF's)
KGE_ERR_BAD_ARG, KGE_ERR_UNSUPPORTED = -3, -4
PKG_NAMES = {"transe": "TransE", "transh": "TransH", "transd": "TransD", "transr": "TransR"}


def adagrad_engine(model, E, R, D, n, nr, alpha=0.01, params=None, Dr=None, use_counts=True, opt="Adagrad", acc0=None):
    """test_gpu_models.make_engine with the initial accumulator settable before the session is made."""
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.use_counts = use_counts
    con.counts_min_records = 0
    con.set_ent_neg_rate(n); con.set_rel_neg_rate(nr); con.set_margin(1.0)
    con.set_opt_method(opt); con.set_alpha(alpha)
    if acc0 is not None:
        con.adagrad_initial_accumulator = acc0
    if Dr is None:
        con.set_dimension(D)
    else:
        con.set_ent_dimension(D); con.set_rel_dimension(Dr); con.hidden_size = D
    hh = np.arange(40) % E
    con.init_from_arrays(E, R, hh, (hh + 1) % E, hh % R)
    con.set_model_and_session(getattr(pkg, PKG_NAMES[model]))
    if params is not None:
        con.set_parameters(params)
    return con


def adagrad_rule_fp32(p, a, g, lr):
    """adagrad_one in numpy fp32: every product, sum, root and quotient rounded once, in its order.  -> (p1, a1, step): a1 is a
    product and a sum and is what the device must hold bit for bit; `step` is (lr g) / sqrt(a1), whose root the device takes
    with the native instruction (within one ulp, not correctly rounded), so p1 is compared through p_allowance.  Elements with
    g == 0 keep p and a, and their step is 0."""
    f = np.float32
    p, a, g = (np.asarray(x, f) for x in (p, a, g))
    nz = g != 0
    a1 = np.where(nz, (a + (g * g).astype(f)).astype(f), a).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        step = np.where(nz, ((f(lr) * g).astype(f) / np.sqrt(a1)).astype(f), f(0)).astype(f)
    return np.where(nz, (p - step).astype(f), p).astype(f), a1, step


def p_allowance(p1, step):
    """How far the device's p1 may lie from adagrad_rule_fp32's (test_gpu_lazy_rows.p_allowance's derivation, without the
    epsilon): the device's root lies within one ulp of the exact one, i.e. within 2^-23 relative, numpy's within half an ulp;
    the exact quotients over the two roots therefore differ by under 1.5 * 2^-23 |step|, and each is rounded once (2^-24
    relative each): together under 2^-22 |step|.  The rounded difference p - step adds one ulp of the result.  Zero where the
    step is zero: an element without gradient must keep every bit."""
    step = np.abs(step).astype(np.float64)
    return np.where(step > 0, 2.0 ** -22 * step + np.spacing(np.abs(p1)).astype(np.float64), 0.0)


def _check_against_rule(got_p, got_a, want_p, want_a, step, what):
    np.testing.assert_array_equal(got_a, want_a, err_msg="accumulator of " + what)
    slack = p_allowance(want_p, step)
    off = np.abs(got_p.astype(np.float64) - want_p)
    assert (off <= slack).all(), ("p of " + what, float((off - slack).max()))


# ---- a. the float-record stage alone --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,D", [("transd", 4), ("transd", 7), ("transe", 50), ("transd", 200), ("transh", 260), ("transh", 1024)])
def test_the_record_stage_alone_against_the_rule(model, D):
    """kge_float_records_apply_adagrad on made-up records (test_gpu_lazy_rows.test_the_apply_stage_alone_bit_for_bit's
    construction: E = 50, R = 3, M = 3000; keys over entity rows, ent_transfer rows and hub copies, keys that carry no record, a
    record of zeros; two calls in a row).  Widths: the float4 ladder's first and last rungs (4, 1024) and 200, the scalar
    ladder's (7, 50), and 260 = 65 float4 units, no multiple of a team.  The accumulators must equal the rule in fp32 numpy BIT
    FOR BIT, on per-row sums taken in record order and hub copies added in copy order; p lies within p_allowance (derivation
    there); rows without a record, and elements whose summed gradient is zero, keep every bit of p and a."""
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    E, R, n_pos_total, n_neg, M = 50, 3, 1000, 1, 3000
    con = adagrad_engine(model, E, R, D, n_neg, 0, use_counts=False)
    names = con.trainModel.table_names
    ent_rows = (2 if model == "transd" else 1) * E
    hub_rows = (1 if model == "transe" else 2) * R
    hub_k = max(1, ((1 if model == "transe" else 2) * n_pos_total) // (hub_rows * 64))
    assert hub_k >= 2
    rows = ent_rows + hub_k * hub_rows
    rng = np.random.default_rng(seed_of(model, D, "adagrad-stage"))
    shapes = [tuple(t.shape) for t in con._tables]
    P = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    A = [(A0 + rng.random(s)).astype(np.float32) for s in shapes]
    tp = [torch.from_numpy(a.copy()).cuda() for a in P]
    ta = [torch.from_numpy(a.copy()).cuda() for a in A]
    zero_elems = bare_rows = 0
    for call in range(2):
        rec = rng.standard_normal((M, D)).astype(np.float32)
        rec[rng.random((M, D)) < 0.2] = 0.0
        rec[:, 0] = 0.0                                                     # element 0 of every row: a zero gradient in a touched row
        rec[M // 2] = 0.0                                                   # a record of zeros
        keys = rng.integers(0, rows, M).astype(np.int32)
        keys[rng.random(M) < 0.5] = rng.integers(ent_rows, rows)            # one hot hub copy: a long run
        keys[rng.random(M) < 0.1] = -1
        keys[:4] = (-7, rows, rows + 5, 2 ** 31 - 1)
        spared = rng.integers(0, rows, 8)                                   # some rows surely without a record
        keys[np.isin(keys, spared)] = -1
        lone = int(keys[M // 2])
        if lone >= 0:                                                       # ... and a row whose ONLY record is the one of zeros
            keys[(keys == lone) & (np.arange(M) != M // 2)] = -1
        lr = 0.01 * (call + 1)
        sums = {}
        for i in np.nonzero((keys >= 0) & (keys < rows))[0]:                # record order within a key
            k = int(keys[i])
            sums[k] = rec[i].copy() if k not in sums else (sums[k] + rec[i]).astype(np.float32)
        want_p, want_a = [a.copy() for a in P], [a.copy() for a in A]
        steps = [np.zeros(a.shape, np.float32) for a in P]

        def apply(t, r, g):
            want_p[t][r], want_a[t][r], steps[t][r] = adagrad_rule_fp32(P[t][r], A[t][r], g, lr)
        for k, g in sums.items():
            if k < E:
                apply(0, k, g)
            elif k < ent_rows:
                apply(3, k - E, g)
        for q in range(hub_rows):
            g, any_ = np.zeros(D, np.float32), False
            for c in range(hub_k):                                          # copy order
                s = sums.get(ent_rows + c * hub_rows + q)
                if s is not None:
                    g, any_ = (g + s).astype(np.float32), True
            if any_:
                apply(1 if q < R else 2, q if q < R else q - R, g)
        d_rec, d_key = torch.from_numpy(rec).cuda(), torch.from_numpy(keys).cuda()
        _lib.check(L.kge_float_records_apply_adagrad(
            ctypes.byref(con._desc), _lib.table_ptrs([t.data_ptr() for t in tp]), _lib.table_ptrs([t.data_ptr() for t in ta]),
            d_rec.data_ptr(), d_key.data_ptr(), M, n_pos_total, n_neg, lr, con._stream()), L)
        torch.cuda.synchronize()
        got_p, got_a = [t.cpu().numpy() for t in tp], [t.cpu().numpy() for t in ta]
        for t, name in enumerate(names):
            _check_against_rule(got_p[t], got_a[t], want_p[t], want_a[t], steps[t], "%s, call %d" % (name, call))
            still = steps[t] == 0                                           # no record, or a zero sum: every bit of both
            np.testing.assert_array_equal(got_p[t][still], P[t][still], err_msg="untouched p of %s, call %d" % (name, call))
            np.testing.assert_array_equal(got_a[t][still], A[t][still], err_msg="untouched a of %s, call %d" % (name, call))
            assert (~still).any(), name
            bare_rows += int(still.all(axis=1).sum())
            zero_elems += int((still & (~still).any(axis=1, keepdims=True)).sum())
        P, A = got_p, want_a                                                # the next call starts from the device's state
    assert zero_elems > 0 and bare_rows > 0                                 # both kinds of untouched element were there


# ---- b. the count-row stage alone ------------------------------------------------------------------------------------------------

def _count_row_call(L, _lib, desc, P, A, d_rows, d_counts, d_n, max_rows, denom, lr):
    from test_gpu_shard_stages import Guarded, _ok
    tabs = [[Guarded(*x.shape).put(x.view(np.int32)) for x in pair] for pair in (P, A)]
    (p, p2), (a, a2) = tabs
    _ok(L.kge_transe_apply_rows_adagrad(ctypes.byref(desc), p.ptr(), p2.ptr(), a.ptr(), a2.ptr(), d_rows.data_ptr(), d_counts.data_ptr(),
                                        d_n.data_ptr(), max_rows, denom, lr, None), _lib)
    return [[g.get().view(np.float32) for g in pair] for pair in tabs]


@pytest.mark.parametrize("dim", [16, 50, 512])
def test_the_count_row_stage_alone_against_the_rule(dim):
    """kge_transe_apply_rows_adagrad on made-up int32 counts over a row list as kge_transe_reduce_records leaves it (entity rows,
    then relation rows; valid row ids behind the list's end that must not be touched).  The row's gradient is the one the
    lazy-Adam call forms -- the normalise-backward of the counts, g = unit / |x| (s - <s, x^> x^) -- so the reference for g is
    that call itself with beta1 = 0 on zero moments, which leaves m = g exactly; the accumulators must then equal the rule in
    fp32 numpy on that g BIT FOR BIT and p lie within p_allowance.  A second table set whose rows are 2^k e_j makes g known in
    closed form, unit 2^-k s off element j and 0 at it (the issue's `(float)count * unit`): the same comparison without the
    helper call.  Unlisted rows, a listed row whose counts are all zero, and zero-gradient elements keep every bit."""
    from test_gpu_shard_stages import Guarded, _desc, _dev, _env, _ok, _row_list
    torch, _lib, L = _env()
    rng = np.random.default_rng(dim + 60)
    E, R, denom, lr = 211, 17, 100, 0.05
    listed, n, d_rows, d_counts, d_n, max_rows = _row_list(rng, E, R, dim)
    counts = d_counts.cpu().numpy().astype(np.int32)
    counts[3] = 0                                           # a listed row without any count
    counts[rng.random(counts.shape) < 0.3] = 0
    counts[:3, 0] = 7
    d_counts = _dev(counts)
    desc = _desc(_lib, E, R, dim)
    unit = np.float32(1.0) / np.float32(denom)

    def start(general):
        out = []
        for rows_ in (E, R):
            if general:
                x = rng.standard_normal((rows_, dim)).astype(np.float32)
            else:
                x = np.zeros((rows_, dim), np.float32)
                x[np.arange(rows_), rng.integers(0, dim, rows_)] = np.ldexp(np.float32(1), rng.integers(-2, 3, rows_)).astype(np.float32)
            out.append(x)
        return out, [(A0 + rng.random((rows_, dim))).astype(np.float32) for rows_ in (E, R)]

    def gradient_from_lazy_adam(P):
        zeros = lambda: [Guarded(*x.shape).put(np.zeros(x.shape, np.int32)) for x in P]
        p, m, v = [Guarded(*x.shape).put(x.view(np.int32)) for x in P], zeros(), zeros()
        _ok(L.kge_transe_apply_rows_adam_lazy(ctypes.byref(desc), p[0].ptr(), p[1].ptr(), m[0].ptr(), m[1].ptr(), v[0].ptr(), v[1].ptr(),
                                              d_rows.data_ptr(), d_counts.data_ptr(), d_n.data_ptr(), max_rows, denom, 0.01, 0.0, 0.999,
                                              1e-8, None, None), _lib)
        return [g.get().view(np.float32) for g in m]         # m = 0 * 0 + g * (1 - 0)

    for general in (True, False):
        P, A = start(general)
        if general:
            G = gradient_from_lazy_adam(P)
        else:
            G = [np.zeros_like(x) for x in P]
            for i, row in enumerate(listed):
                t, r = (0, row) if row < E else (1, row - E)
                j = int(np.nonzero(P[t][r])[0][0])
                inv = np.float32(1.0) / P[t][r, j]
                G[t][r] = (unit * inv) * counts[i].astype(np.float32)           # exact scalings by a power of two, then one product
                G[t][r, j] = 0.0
        got_p, got_a = _count_row_call(L, _lib, desc, P, A, d_rows, d_counts, d_n, max_rows, denom, lr)
        for t, what in enumerate(("entity table", "relation table")):
            want_p, want_a, step = adagrad_rule_fp32(P[t], A[t], G[t], lr)
            _check_against_rule(got_p[t], got_a[t], want_p, want_a, step, "%s, dim %d, general %s" % (what, dim, general))
            moved = listed[listed < E] if t == 0 else listed[listed >= E] - E
            kept = np.setdiff1d(np.arange(P[t].shape[0]), moved)
            assert not G[t][kept].any() and G[t][moved].any(axis=1).sum() >= len(moved) - 1
            np.testing.assert_array_equal(got_p[t][kept], P[t][kept])
            np.testing.assert_array_equal(got_a[t][kept], A[t][kept])
            still = G[t] == 0
            assert t == 1 or still[moved].any()
            np.testing.assert_array_equal(got_p[t][still], P[t][still])
            np.testing.assert_array_equal(got_a[t][still], A[t][still])
        r3 = int(listed[3])
        assert r3 < E and not G[0][r3].any()


# ---- c. the dense sweep ------------------------------------------------------------------------------------------------------------

SWEEP_SHAPES = [(7, 5), (33, 50), (301, 50), (9, 11)]       # 35, 1650, 15050 and 99 elements: none a multiple of 4; 15 blocks for the third


def _sweep_inputs(rng, shapes):
    P = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    A = [(A0 + rng.random(s)).astype(np.float32) for s in shapes]
    G = []
    for s in shapes:
        g = rng.standard_normal(s).astype(np.float32)
        g[rng.random(s) < 0.4] = 0.0
        flat = g.reshape(-1)
        flat[8:24] = 0.0                                     # whole 16-byte groups without gradient
        flat[-1] = 0.5                                       # ... and the scalar tail has one
        flat[-2] = 0.0
        G.append(g)
    return P, A, G


def _sweep(L, _lib, P, A, G, lr):
    import torch
    dev = lambda arrs: [torch.from_numpy(a.copy()).cuda() for a in arrs]
    tp, ta, tg = dev(P), dev(A), dev(G)
    numel = (ctypes.c_int64 * 4)(*[t.numel() for t in tp])
    ptrs = lambda ts: _lib.table_ptrs([t.data_ptr() for t in ts])
    _lib.check(L.kge_adagrad_update_tables(len(tp), ptrs(tp), ptrs(ta), ptrs(tg), numel, lr, None), L)
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in ts] for ts in (tp, ta, tg)]


def test_the_dense_sweep_against_the_rule():
    """kge_adagrad_update_tables over four tables whose element counts are no multiples of 4 (the scalar tail runs) and, for one,
    more than a block's worth: accumulators bit for bit, p within p_allowance, elements and whole 16-byte groups without
    gradient untouched, the gradient zero afterwards."""
    from openkeonspark_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(77)
    P, A, G = _sweep_inputs(rng, SWEEP_SHAPES)
    got_p, got_a, got_g = _sweep(L, _lib, P, A, G, 0.03)
    for t, s in enumerate(SWEEP_SHAPES):
        assert (s[0] * s[1]) % 4 and not G[t].reshape(-1)[8:24].any()
        want_p, want_a, step = adagrad_rule_fp32(P[t], A[t], G[t], 0.03)
        _check_against_rule(got_p[t], got_a[t], want_p, want_a, step, "table %d" % t)
        still = G[t] == 0
        np.testing.assert_array_equal(got_p[t][still], P[t][still])
        np.testing.assert_array_equal(got_a[t][still], A[t][still])
        assert (got_p[t][~still] != P[t][~still]).any() and not got_g[t].any()


# ---- d. touched rows == dense sweep ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [16, 50])
def test_touched_rows_equal_the_dense_sweep(D):
    """The feature's claim.  One starting state of TransD's four tables; a gradient with one record per row for most rows (so a
    row's sum IS its record; relation-side rows through hub copy 0) goes through kge_float_records_apply_adagrad, and as dense
    gradient tables through kge_adagrad_update_tables: p and a must come out equal BIT FOR BIT -- both run adagrad_one -- and
    the rows without a record keep every bit in both."""
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    E, R, n_pos_total = 50, 3, 1000
    con = adagrad_engine("transd", E, R, D, 1, 0)
    rng = np.random.default_rng(D + 90)
    shapes = [tuple(t.shape) for t in con._tables]
    P = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    A = [(A0 + rng.random(s)).astype(np.float32) for s in shapes]
    G = [np.zeros(s, np.float32) for s in shapes]
    keys, recs = [], []
    ent_rows = 2 * E
    for key in range(ent_rows + 2 * R):
        if rng.random() < 0.25 and key not in (0, ent_rows):
            continue                                         # a row without a record
        g = rng.standard_normal(D).astype(np.float32)
        g[rng.random(D) < 0.3] = 0.0
        if key < E: G[0][key] = g
        elif key < ent_rows: G[3][key - E] = g
        elif key < ent_rows + R: G[1][key - ent_rows] = g
        else: G[2][key - ent_rows - R] = g
        keys.append(key); recs.append(g)
    keys += [-1, -1]; recs += [np.ones(D, np.float32)] * 2
    order = rng.permutation(len(keys))
    keys, recs = np.array(keys, np.int32)[order], np.stack(recs)[order]
    dev = lambda arrs: [torch.from_numpy(a.copy()).cuda() for a in arrs]
    tp, ta = dev(P), dev(A)
    d_rec, d_key = torch.from_numpy(recs).cuda(), torch.from_numpy(keys).cuda()
    _lib.check(L.kge_float_records_apply_adagrad(
        ctypes.byref(con._desc), _lib.table_ptrs([t.data_ptr() for t in tp]), _lib.table_ptrs([t.data_ptr() for t in ta]),
        d_rec.data_ptr(), d_key.data_ptr(), len(keys), n_pos_total, 1, 0.02, con._stream()), L)
    torch.cuda.synchronize()
    dense_p, dense_a, _ = _sweep(L, _lib, P, A, G, 0.02)
    n_bare = 0
    for t, name in enumerate(con.trainModel.table_names):
        np.testing.assert_array_equal(tp[t].cpu().numpy(), dense_p[t], err_msg="p of " + name)
        np.testing.assert_array_equal(ta[t].cpu().numpy(), dense_a[t], err_msg="a of " + name)
        bare = ~G[t].any(axis=1)
        n_bare += int(bare.sum())
        np.testing.assert_array_equal(dense_p[t][bare], P[t][bare])
        np.testing.assert_array_equal(dense_a[t][bare], A[t][bare])
        assert (dense_a[t][~bare] != A[t][~bare]).any()
    assert n_bare > 0


# ---- e. whole steps against the oracle's gradient ----------------------------------------------------------------------------------

def _clean_batch(model, orc, p0, make, B, N, De, Dr, nr, tries=40):
    """test_gpu_lazy_rows.clean_batch for any (De, Dr)."""
    from torch_ref import near_kink_rows
    for i in range(tries):
        bh, bt, br = make()
        if np.abs(orc.hinge_margins(bh, bt, br, B, N)).min() <= 1e-4:
            continue
        if near_kink_rows(model, p0, bh, bt, br, B, N, De, Dr, tol=1e-6, negative_rel=nr)[1] == 0:
            return bh, bt, br, i
    raise AssertionError("no batch without ties and near-zero elements in %d draws" % tries)


def _state(con):
    names = con.trainModel.table_names
    return con.get_parameters(), {k: con._adagrad_acc[i].cpu().numpy() for i, k in enumerate(names)}


def adagrad_step_against_the_rule(con, orc, bh, bt, br, B, N, alpha):
    """One hand-fed step against the rule on the oracle's gradient g_o, from the state both start from.  The device's gradient
    is held to the parity bar: within d = RTOL max|g_o| of g_o per element.
      rows the step does not touch: p and a bit for bit;
      a on touched rows: a0 + g^2 over that interval is within 2 |g_o| d + d^2 of a0 + g_o^2, plus two fp32 ulps of the result
        (the product's and the sum's roundings) -- the bound LazyAdam's v gets, without its (1 - beta2);
      p on touched rows: the step s(g) = lr g / sqrt(a0 + g^2) rises with g (ds/dg = lr a0 / (a0 + g^2)^1.5 > 0), so the update
        p1 - p0 lies in [-s(g_o + d), -s(g_o - d)], evaluated in fp64, widened by 2^-21 of the larger end (five roundings of the
        fp32 evaluation -- g*g and the sum, halved by the root, the root's own ulp, lr*g and the quotient: under 5 * 2^-24) and
        one ulp of the larger of |p0|, |p1| (the rounding of p0 - step).  s(0) = 0: an element one side takes for zero is inside.
    -> number of touched rows checked."""
    names = con.trainModel.table_names
    p0, a0 = _state(con)
    orc.params = {k: v.copy() for k, v in p0.items()}
    active = orc.hinge_margins(bh, bt, br, B, N) > 0
    loss_o, g_o = orc.grad(bh, bt, br, B, N)
    touched = touched_rows(names, active, bh, bt, br, B)
    loss_g = con.train_step(bh, bt, br, None)
    assert abs(loss_g - loss_o) <= 2e-5 * abs(loss_o), (loss_g, loss_o)
    p1, a1 = _state(con)
    lr = float(np.float32(alpha))
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    checked = 0
    for k in names:
        T = touched[k]
        rest = np.setdiff1d(np.arange(p0[k].shape[0]), T)
        np.testing.assert_array_equal(p1[k][rest], p0[k][rest], err_msg=k)
        np.testing.assert_array_equal(a1[k][rest], a0[k][rest], err_msg=k)
        assert (g_o[k][rest] == 0).all(), k
        if not len(T):
            continue
        pT, aT, gT = (x[T].astype(np.float64) for x in (p0[k], a0[k], g_o[k]))
        d = RTOL * np.abs(g_o[k]).max()
        a_exp = aT + gT * gT
        da = np.abs(a1[k][T] - a_exp) - (2 * np.abs(gT) * d + d * d + 2 * ulp(a_exp))
        assert (da <= 0).all(), (k, "a", float(da.max()))
        s = lambda g: lr * g / np.sqrt(aT + g * g)
        s_lo, s_hi = s(gT - d), s(gT + d)
        w = 2.0 ** -21 * np.maximum(np.abs(s_lo), np.abs(s_hi)) + ulp(np.maximum(np.abs(p0[k][T]), np.abs(p1[k][T])))
        du = p1[k][T].astype(np.float64) - pT
        dp = np.maximum(du - (-s_lo + w), (-s_hi - w) - du)
        assert (dp <= 0).all(), (k, "p", float(dp.max()))
        assert (a1[k][T] != a0[k][T]).any() and (p1[k][T] != p0[k][T]).any(), k
        checked += len(T)
    return checked


def run_adagrad_steps(model, E, R, D, B, n, nr, steps, use_counts=True, alpha=0.01, Dr=None, tag=""):
    Dr_ = D if Dr is None else Dr
    rng = np.random.default_rng(seed_of(model, E, R, D, B, n, nr, "adagrad"))
    params = oracle.init_params(oracle.MODEL_IDS[model], E, R, D, Dr_, seed=8)
    orc = oracle.Model(model, E, R, D, Dr_, margin=1.0, negative_rel=nr, params=params)
    con = adagrad_engine(model, E, R, D, n, nr, alpha=alpha, params=params, Dr=Dr, use_counts=use_counts)
    assert con._adagrad and not con._has_slots and not con.persistent_supported()
    assert len(con._adagrad_acc) == len(con.trainModel.table_names)
    assert all(float(a.min()) == float(a.max()) == float(np.float32(A0)) and a.shape == t.shape for a, t in zip(con._adagrad_acc, con._tables))
    checked = redraws = 0
    for step in range(steps):
        orc.params = con.get_parameters()
        bh, bt, br, i = _clean_batch(model, orc, orc.params, lambda: rand_batch(rng, E, R, B, n, nr, distinct=True), B, n + nr, D, Dr_, nr)
        redraws += i
        checked += adagrad_step_against_the_rule(con, orc, bh, bt, br, B, n + nr, alpha)
    assert checked > 0 and con.global_step == steps
    parity_report("adagrad_%s%s" % (model, tag), touched_rows_checked=checked, steps=steps, redraws=redraws, rows_excused=0)
    return con, orc, rng


@pytest.mark.parametrize("model,use_counts,n,nr", [("transe", True, 3, 0), ("transe", False, 2, 1), ("transh", True, 3, 0),
                                                   ("transd", True, 3, 0)])
def test_adagrad_steps_follow_the_rule_on_the_oracle_gradient(model, use_counts, n, nr):
    """Four hand-fed steps at test_gpu_lazy_rows.run_steps' shape over all tables of the model: TransE on the sign-count path
    (reduce, then kge_transe_apply_rows_adagrad) and off it with a relation negative, TransH and TransD from float records
    (kge_forward_backward_adagrad_rows).  No gradient tables exist on any of them."""
    con, _, _ = run_adagrad_steps(model, 400, 40, 64, 96, n, nr, 4, use_counts=use_counts, tag="_n%d_nr%d_c%d" % (n, nr, use_counts))
    assert con._grads == []
    if model == "transe" and use_counts:
        assert con.sparse_rows and not con.sparse_inplace
    else:
        assert con.sparse_inplace and not con.sparse_rows


@pytest.mark.parametrize("model", ["transh", "transd"])
def test_adagrad_steps_with_hub_copies(model):
    """R = 2, B = 256: the four relation-side rows are spread over hub copies, which hub_fold_adam_kernel adds in copy order
    before the rule is applied once per row."""
    con, _, _ = run_adagrad_steps(model, 300, 2, 16, 256, 1, 0, 4, tag="_hub")
    assert con._grads == [] and con.sparse_inplace


def test_adagrad_steps_of_transr_through_the_dense_sweep():
    """TransR keeps its dense gradient tables in one process; apply_gradients ends in kge_adagrad_update_tables, which leaves
    the gradient tables zero for the next step."""
    con, _, _ = run_adagrad_steps("transr", 120, 9, 12, 64, 3, 0, 4, Dr=8)
    assert len(con._grads) == len(con._tables) and not con.sparse_rows and not con.sparse_inplace
    assert not any(g.any().item() for g in con._grads)


# ---- f. errors -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("acc0", [0, -1])
def test_a_non_positive_initial_accumulator_is_refused(acc0):
    import openkeonspark_amd as pkg
    with pytest.raises(pkg.KgeError, match="adagrad_initial_accumulator"):
        adagrad_engine("transh", 60, 4, 16, 1, 0, acc0=acc0)
    con = adagrad_engine("transh", 60, 4, 16, 1, 0, acc0=-1, opt="SGD")          # (only Adagrad reads it)
    assert not con._adagrad


def test_errors_of_the_adagrad_entry_points():
    import torch
    import openkeonspark_amd as pkg
    from openkeonspark_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)

    def batch(con, E, R, B):
        bh, bt, br = rand_batch(rng, E, R, B, 1, 0, distinct=True)
        return torch.from_numpy(np.stack([bh, bt, br]).astype(np.int32)).cuda()

    def refused(call, code, watched):
        before = [t.clone() for t in watched]
        rc = call()
        torch.cuda.synchronize()
        assert rc == code, (rc, _lib.last_error(L))
        L.kge_clear_error()
        for t, b in zip(watched, before):
            assert torch.equal(t, b)

    # a missing accumulator: KGE_ERR_BAD_ARG before anything is launched
    con = adagrad_engine("transd", 60, 4, 16, 1, 0)
    dev = batch(con, 60, 4, 32)
    acc = [t.data_ptr() for t in con._adagrad_acc]
    holes = _lib.table_ptrs(acc[:2] + [None] + acc[3:])
    watched = list(con._tables) + list(con._adagrad_acc)
    rec, key = torch.ones((8, 16), device="cuda"), torch.arange(8, dtype=torch.int32, device="cuda")
    for ptrs in (holes, None):
        refused(lambda: L.kge_forward_backward_adagrad_rows(
            ctypes.byref(con._desc), con._tab_ptrs, ptrs, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 32, 1, 32, 32, 0.01,
            con._loss.data_ptr(), con._stream()), KGE_ERR_BAD_ARG, watched)
        refused(lambda: L.kge_float_records_apply_adagrad(
            ctypes.byref(con._desc), con._tab_ptrs, ptrs, rec.data_ptr(), key.data_ptr(), 8, 32, 1, 0.01, con._stream()),
            KGE_ERR_BAD_ARG, watched)
    grads = [torch.ones_like(t) for t in con._tables]
    for ptrs in (holes, None):
        refused(lambda: L.kge_adagrad_update_tables(4, con._tab_ptrs, ptrs, _lib.table_ptrs([g.data_ptr() for g in grads]), con._numel, 0.01,
                                                    con._stream()), KGE_ERR_BAD_ARG, watched + grads)
    cte = adagrad_engine("transe", 60, 4, 16, 1, 0)
    rows, counts, n1 = (torch.zeros(4, dtype=torch.int32, device="cuda"), torch.ones((4, 16), dtype=torch.int32, device="cuda"),
                        torch.ones(1, dtype=torch.int32, device="cuda"))
    for a_ent, a_rel in ((cte._adagrad_acc[0].data_ptr(), None), (None, cte._adagrad_acc[1].data_ptr())):
        refused(lambda: L.kge_transe_apply_rows_adagrad(
            ctypes.byref(cte._desc), cte._tables[0].data_ptr(), cte._tables[1].data_ptr(), a_ent, a_rel, rows.data_ptr(), counts.data_ptr(),
            n1.data_ptr(), 4, 32, 0.01, cte._stream()), KGE_ERR_BAD_ARG, list(cte._tables) + list(cte._adagrad_acc))
    # TransR has no record path: the row entry points say so, the tables stay
    ctr = adagrad_engine("transr", 60, 4, 16, 1, 0, Dr=8)
    dev = batch(ctr, 60, 4, 32)
    watched = list(ctr._tables) + list(ctr._adagrad_acc)
    refused(lambda: L.kge_forward_backward_adagrad_rows(
        ctypes.byref(ctr._desc), ctr._tab_ptrs, ctr._adagrad_ptrs, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 32, 1, 32, 32,
        0.01, ctr._loss.data_ptr(), ctr._stream()), KGE_ERR_UNSUPPORTED, watched)
    refused(lambda: L.kge_float_records_apply_adagrad(
        ctypes.byref(ctr._desc), ctr._tab_ptrs, ctr._adagrad_ptrs, rec.data_ptr(), key.data_ptr(), 8, 32, 1, 0.01, ctr._stream()),
        KGE_ERR_UNSUPPORTED, watched)
    # no persistent launch, on any path
    for c in (con, cte, ctr):
        assert not c.persistent_supported()
        with pytest.raises(pkg.KgeError, match="persistent"):
            c.train_steps(2, persistent=True)
    small = adagrad_engine("transe", 60, 4, 16, 1, 0, use_counts=False)
    assert small.sparse_inplace and not small.persistent_supported()
    # negatives that are not single-slot corruptions: the existing error of the in-place step
    for model, nr in (("transh", 0), ("transh", 1)):
        c = adagrad_engine(model, 300, 7, 64, 3, nr)
        bh, bt, br = rand_batch(rng, 300, 7, 160, 3, nr, foreign=0.3 if nr == 0 else 0.0, distinct=True)
        with pytest.raises(pkg.KgeError, match="single-slot"):
            c.train_step(bh, bt, br, None)
    # the optimizers beside it keep their refusals
    with pytest.raises(pkg.KgeError, match="TransR"):
        adagrad_engine("transr", 60, 4, 16, 1, 0, Dr=8, opt="LazyAdam")


# ---- g. reproducibility ------------------------------------------------------------------------------------------------------------

def _train_kg_small(model_name, steps):
    import openkeonspark_amd as pkg
    pkg._lib.lib().kge_set_option(b"libc_rand_restart", 1)                  # the sampler's seeds as in a new process
    con = pkg.Config()
    con.set_in_path(os.path.join(GOLDEN, "kg_small"))
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(48); con.set_nbatches(10)      # B = 600
    con.set_ent_neg_rate(3); con.set_rel_neg_rate(0); con.set_alpha(0.05); con.set_opt_method("Adagrad")
    con.counts_min_records = 0
    con.init()
    con.set_model_and_session(getattr(pkg, model_name))
    assert con._adagrad and (con.sparse_rows or con.sparse_inplace) and con._grads == []
    losses = [con.train_step() for _ in range(steps)]
    return losses, _state(con)


@pytest.mark.parametrize("model_name", ["TransH", "TransE"])
def test_adagrad_training_is_reproducible_bit_for_bit(model_name):
    """Two runs from the same parameters and the same sampled batches: no sum of the step depends on scheduling, so losses,
    tables and accumulators agree in every bit."""
    a = _train_kg_small(model_name, 12)
    b = _train_kg_small(model_name, 12)
    assert a[0] == b[0]
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert all(np.isfinite(a[0]))
    assert all(v.min() >= np.float32(A0) and v.max() > np.float32(A0) for v in a[1][1].values())
