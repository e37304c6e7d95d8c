"""opt_method "RowAdagrad": row-wise Adagrad (PyTorch-BigGraph's RowAdagrad) on the touched-rows paths (TransE sign counts,
TransE / TransH / TransD float records) and on dense gradient tables (TransR).  ONE fp32 accumulator per table row; per row of
length L, in fp32 (csrc/optim_dev.hpp):

    q = sum_j g[j]^2;  a = a + q / L;  s = sqrt(a);  p[j] = p[j] - (lr g[j]) / s   where g[j] != 0

no epsilon, accumulators from Config.adagrad_initial_accumulator (0.1).  A row whose gradient is all zero keeps p and a bit for
bit, and so does an element with g = 0 in a row that moves: "only the touched rows" is the dense rule.

Each stage alone against the rule in fp64 numpy on a gradient the test supplies (a_allowance / p_allowance below: derived, not
fitted), whole steps against the rule on the CPU oracle's gradient, one shared-negatives step per model checked by the existing
shared-step modules' own references, reproducibility, and the refusals.  Ranks: tests/test_gpu_row_adagrad_dp.py; the driver
and checkpoints: tests/test_gpu_row_adagrad_checkpoint.py; the plan and the checkpoint files: tests/test_row_adagrad_plan.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity_report
from oracle import oracle
from test_gpu_adagrad import A0, KGE_ERR_BAD_ARG, KGE_ERR_UNSUPPORTED, _clean_batch, adagrad_engine
from test_gpu_lazy_rows import RTOL, touched_rows
from test_gpu_models import rand_batch, seed_of

pytestmark = pytest.mark.gpu

OPT = "RowAdagrad"


def engine(model, E, R, D, n, nr, **kw):
    con = adagrad_engine(model, E, R, D, n, nr, opt=OPT, **kw)
    assert con._row_adagrad and con._rows_rule and not con._adagrad and not con._has_slots
    return con


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def row_rule_fp64(p, a, g, lr):
    """The rule in fp64 on fp32 inputs: p, g [n, L], a [n].  -> (p1, a1, inc, step) in fp64; inc = q / L, step = lr g / sqrt(a1)
    (zero where g is zero: such an element keeps its p; a row of zeros has inc = 0 and a1 = a exactly)."""
    p, a, g = (np.asarray(x, np.float32).astype(np.float64) for x in (p, a, g))
    inc = (g * g).sum(axis=1) / g.shape[1]
    a1 = a + inc
    step = float(np.float32(lr)) * g / np.sqrt(a1)[:, None]
    return p - step, a1, inc, step


def a_allowance(a1, inc, L):
    """How far the device's accumulator may lie from row_rule_fp64's.  The device forms q / L from L squares (each rounded once:
    2^-24 relative), L - 1 adds in an order of its own (each rounds a partial sum that is at most q, all terms being >= 0: 2^-24 q
    each) and one divide (2^-24): to first order (L + 2) 2^-24 of the increment, widened by the factor 1 + (L + 2) 2^-24 for the
    products of those terms.  The closing add a + q / L rounds the result once: half an ulp of it.  A row of zeros: exactly 0."""
    e = (L + 2) * 2.0 ** -24
    return np.where(inc > 0, e * (1 + e) * inc + 0.5 * ulp32(a1), 0.0)


def p_allowance(p0, p1, step, a1, da):
    """... and p.  An accumulator off by da moves the root by da / (2 a1) relative; the device's root is the native instruction's
    (within one ulp, 2^-23 relative), lr g and the quotient are rounded once each (2^-24 each): the step is within
    da / (2 a1) + 2^-22 of row_rule_fp64's, relative, widened by 1 + 2^-20 for the products of the terms (each is below 2^-8 at
    every shape here).  The difference p - step is rounded once: within one ulp of the larger of |p0|, |p1|.  Zero where the step
    is zero: an element without gradient keeps every bit."""
    rel = (da / (2 * a1))[:, None] + 2.0 ** -22
    step = np.abs(step)
    return np.where(step > 0, rel * (1 + 2.0 ** -20) * step + ulp32(np.maximum(np.abs(p0), np.abs(p1))), 0.0)


def check_against_rule(got_p, got_a, p0, a0, g, lr, what):
    """The device's p [n, L] and a [n] against the rule from (p0, a0) on g.  -> the elements whose step is zero."""
    L = g.shape[1]
    want_p, want_a, inc, step = row_rule_fp64(p0, a0, g, lr)
    da = a_allowance(want_a, inc, L)
    off_a = np.abs(got_a.astype(np.float64) - want_a)
    assert (off_a <= da).all(), ("accumulator of " + what, float((off_a - da).max()))
    slack = p_allowance(p0.astype(np.float64), want_p, step, want_a, da)
    off_p = np.abs(got_p.astype(np.float64) - want_p)
    assert (off_p <= slack).all(), ("p of " + what, float((off_p - slack).max()))
    still = step == 0
    np.testing.assert_array_equal(got_p[still], p0[still], err_msg="zero-gradient elements of " + what)
    bare = ~(g != 0).any(axis=1)
    np.testing.assert_array_equal(got_a[bare], a0[bare], err_msg="accumulators of the rows without gradient of " + what)
    assert (got_a[~bare] > a0[~bare]).all(), what
    return still


# ---- a. the float-record stage alone --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,D", [("transd", 4), ("transd", 7), ("transe", 50), ("transd", 200), ("transh", 260), ("transh", 1024)])
def test_the_record_stage_alone_against_the_rule(model, D):
    """kge_float_records_apply_rowadagrad on made-up records: tests/test_gpu_adagrad.py
    test_the_record_stage_alone_against_the_rule's construction (E = 50, R = 3, M = 3000; keys over entity rows, ent_transfer
    rows and hub copies, keys that carry no record, a record of zeros, one hot hub copy, two calls in a row).  Widths: the float4
    ladder's first and last rungs (4, 1024) and 200, the scalar ladder's (7, 50 -- lanes that hold no element), and 260 = 65
    float4 units, no multiple of a team.  g is the per-row sum in record order, hub copies added in copy order, formed here in
    fp32 as the device forms it; the rule on it in fp64, within a_allowance / p_allowance."""
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    E, R, n_pos_total, n_neg, M = 50, 3, 1000, 1, 3000
    con = engine(model, E, R, D, n_neg, 0, use_counts=False)
    names = con.trainModel.table_names
    ent_rows = (2 if model == "transd" else 1) * E
    hub_rows = (1 if model == "transe" else 2) * R
    hub_k = max(1, ((1 if model == "transe" else 2) * n_pos_total) // (hub_rows * 64))
    assert hub_k >= 2
    rows = ent_rows + hub_k * hub_rows
    rng = np.random.default_rng(seed_of(model, D, "rowadagrad-stage"))
    shapes = [tuple(t.shape) for t in con._tables]
    assert [tuple(a.shape) for a in con._rowadagrad_acc] == [(s[0],) for s in shapes]
    P = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    A = [(A0 + rng.random(s[0])).astype(np.float32) for s in shapes]
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
        G = [np.zeros(s, np.float32) for s in shapes]
        for k, g in sums.items():
            if k < E:
                G[0][k] = g
            elif k < ent_rows:
                G[3][k - E] = g
        for q in range(hub_rows):
            g, any_ = np.zeros(D, np.float32), False
            for c in range(hub_k):                                          # copy order
                s = sums.get(ent_rows + c * hub_rows + q)
                if s is not None:
                    g, any_ = (g + s).astype(np.float32), True
            if any_:
                G[1 if q < R else 2][q if q < R else q - R] = g
        d_rec, d_key = torch.from_numpy(rec).cuda(), torch.from_numpy(keys).cuda()
        _lib.check(L.kge_float_records_apply_rowadagrad(
            ctypes.byref(con._desc), _lib.table_ptrs([t.data_ptr() for t in tp]), _lib.table_ptrs([t.data_ptr() for t in ta]),
            d_rec.data_ptr(), d_key.data_ptr(), M, n_pos_total, n_neg, lr, con._stream()), L)
        torch.cuda.synchronize()
        got_p, got_a = [t.cpu().numpy() for t in tp], [t.cpu().numpy() for t in ta]
        for t, name in enumerate(names):
            still = check_against_rule(got_p[t], got_a[t], P[t], A[t], G[t], lr, "%s, call %d" % (name, call))
            assert (~still).any(), name
            bare_rows += int(still.all(axis=1).sum())
            zero_elems += int((still & (~still).any(axis=1, keepdims=True)).sum())
        P, A = got_p, got_a                                                 # the next call starts from the device's state
    assert zero_elems > 0 and bare_rows > 0                                 # both kinds of untouched element were there


# ---- b. the listed-rows stage alone ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [16, 50, 512])
def test_the_listed_rows_stage_alone_against_the_rule(dim):
    """kge_transe_apply_rows_rowadagrad on made-up int32 counts over a row list as kge_transe_reduce_records leaves it:
    tests/test_gpu_adagrad.py test_the_count_row_stage_alone_against_the_rule's shapes and construction.  The row's gradient is
    the one the lazy-Adam call forms (the normalise-backward of the counts), so the reference for g is that call itself with
    beta1 = 0 on zero moments, which leaves m = g exactly; a second table set whose rows are 2^k e_j makes g known in closed form.
    The rule on that g in fp64, within a_allowance / p_allowance.  Unlisted rows (valid ids behind the list's end among them), a
    listed row whose counts are all zero and zero-gradient elements keep every bit; nothing is written outside the arrays."""
    from test_gpu_shard_stages import Guarded, _desc, _dev, _env, _ok, _row_list
    torch, _lib, L = _env()
    rng = np.random.default_rng(dim + 160)
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
        return out, [(A0 + rng.random(rows_)).astype(np.float32) for rows_ in (E, R)]

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
        tabs = [[Guarded(*x.shape).put(x.view(np.int32)) for x in pair] for pair in (P, A)]
        (p, p2), (a, a2) = tabs
        _ok(L.kge_transe_apply_rows_rowadagrad(ctypes.byref(desc), p.ptr(), p2.ptr(), a.ptr(), a2.ptr(), d_rows.data_ptr(),
                                               d_counts.data_ptr(), d_n.data_ptr(), max_rows, denom, lr, None), _lib)
        got_p, got_a = [[g.get().view(np.float32) for g in pair] for pair in tabs]
        for t, what in enumerate(("entity table", "relation table")):
            still = check_against_rule(got_p[t], got_a[t], P[t], A[t], G[t], lr, "%s, dim %d, general %s" % (what, dim, general))
            moved = listed[listed < E] if t == 0 else listed[listed >= E] - E
            kept = np.setdiff1d(np.arange(P[t].shape[0]), moved)
            assert not G[t][kept].any() and G[t][moved].any(axis=1).sum() >= len(moved) - 1
            np.testing.assert_array_equal(got_p[t][kept], P[t][kept])
            np.testing.assert_array_equal(got_a[t][kept], A[t][kept])
            assert t == 1 or still[moved].any()
            assert (got_p[t][moved] != P[t][moved]).any()
        r3 = int(listed[3])
        assert r3 < E and not G[0][r3].any() and got_a[0][r3] == A[0][r3]


# ---- c. the dense stage alone ------------------------------------------------------------------------------------------------------

# Row counts 1, 3 and 70 (a wave per row: 70 rows are 18 workgroups, the last half empty), row lengths 1 and 6 (scalar accesses,
# lanes without an element), 200 (float4, one pass of a wave), 40 000 (a 200 x 200 matrix: the workgroup, 40 passes) and 1030
# (beyond 1024 and no multiple of 4: the workgroup with scalar accesses); one to four tables per call.
DENSE_CALLS = [[(70, 1), (3, 6), (70, 200), (3, 40000)], [(1, 40000), (1, 6), (3, 1030)], [(70, 6)], [(3, 200), (1, 1)]]


@pytest.mark.parametrize("shapes", DENSE_CALLS, ids=lambda s: "+".join("%dx%d" % x for x in s))
def test_the_dense_stage_alone_against_the_rule(shapes):
    """kge_rowadagrad_update_tables on gradient tables with some rows zero and zero elements in the others: the rule in fp64
    within a_allowance / p_allowance (at 40 000 elements the sum of squares runs over four waves and 40 passes); rows without
    gradient keep p and a bit for bit; the gradient is zero afterwards; nothing is written outside the arrays."""
    from test_gpu_shard_stages import Guarded, _env, _ok
    torch, _lib, L = _env()
    rng = np.random.default_rng(seed_of("rowadagrad-dense", len(shapes), shapes[0][1]))
    lr = 0.03
    P = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    A = [(A0 + rng.random(s[0])).astype(np.float32) for s in shapes]
    G = []
    for rows, length in shapes:
        g = rng.standard_normal((rows, length)).astype(np.float32)
        if length > 1:
            g[rng.random((rows, length)) < 0.4] = 0.0
            g[:, length // 2] = 0.5                              # (no row is zero by chance)
        if length >= 16:
            g[:, 4:12] = 0.0                                     # whole 16-byte groups without gradient in a row that moves
        if rows > 1:
            g[rng.choice(rows, max(1, rows // 3), replace=False)] = 0.0      # rows without gradient
        G.append(g)
    tabs = [[Guarded(*x.shape).put(x.view(np.int32)) for x in arrs] for arrs in (P, A, G)]
    ptrs = lambda ts: _lib.table_ptrs([t.ptr() for t in ts])
    rows_ = (ctypes.c_int64 * 4)(*[s[0] for s in shapes])
    lens_ = (ctypes.c_int64 * 4)(*[s[1] for s in shapes])
    _ok(L.kge_rowadagrad_update_tables(len(shapes), ptrs(tabs[0]), ptrs(tabs[1]), ptrs(tabs[2]), rows_, lens_, lr, None), _lib)
    got_p, got_a, got_g = [[g.get().view(np.float32) for g in ts] for ts in tabs]
    n_bare = 0
    for t, s in enumerate(shapes):
        check_against_rule(got_p[t], got_a[t], P[t], A[t], G[t], lr, "table %d %s" % (t, s))
        bare = ~G[t].any(axis=1)
        n_bare += int(bare.sum())
        np.testing.assert_array_equal(got_p[t][bare], P[t][bare])
        assert not got_g[t].any() and (got_p[t][~bare] != P[t][~bare]).any()
    assert n_bare > 0 or all(s[0] == 1 for s in shapes)


# ---- d. whole steps against the oracle's gradient ----------------------------------------------------------------------------------

def _state(con):
    names = con.trainModel.table_names
    return con.get_parameters(), {k: con._rowadagrad_acc[i].cpu().numpy() for i, k in enumerate(names)}


def step_against_the_rule(con, orc, bh, bt, br, B, N, alpha):
    """One hand-fed step against the rule on the oracle's gradient g_o, from the state both start from:
    tests/test_gpu_adagrad.py adagrad_step_against_the_rule's construction and its bar on the device's gradient, within
    d = RTOL max|g_o| of g_o per element.
      rows the step does not touch: p and a bit for bit;
      a on touched rows: the increment mean(g^2) lies between mean(max(|g_o| - d, 0)^2) and mean((|g_o| + d)^2); a1 lies between
        a0 + those, widened by a_allowance of the upper end (plus the other half ulp: the ends are not the rounded value);
      p on touched rows: the step lr g / sqrt(a1) rises with g and falls with a1, so the update p1 - p0 lies between
        -max_a lr (g_o + d) / sqrt(a) and -min_a lr (g_o - d) / sqrt(a) over the two ends of a1 (a superset: g's own share of a1
        is not tied to it), evaluated in fp64 and widened as p_allowance widens.  An element one side takes for zero is inside.
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
    checked = 0
    for k in names:
        T = touched[k]
        rest = np.setdiff1d(np.arange(p0[k].shape[0]), T)
        np.testing.assert_array_equal(p1[k][rest], p0[k][rest], err_msg=k)
        np.testing.assert_array_equal(a1[k][rest], a0[k][rest], err_msg=k)
        assert (g_o[k][rest] == 0).all(), k
        if not len(T):
            continue
        L = p0[k].shape[1]
        pT, aT, gT = (x[T].astype(np.float64) for x in (p0[k], a0[k], g_o[k].reshape(p0[k].shape)))
        d = RTOL * np.abs(g_o[k]).max()
        inc_lo = (np.maximum(np.abs(gT) - d, 0) ** 2).sum(axis=1) / L
        inc_hi = ((np.abs(gT) + d) ** 2).sum(axis=1) / L
        a_lo, a_hi = aT + inc_lo, aT + inc_hi
        ea = a_allowance(a_hi, inc_hi, L) + 0.5 * ulp32(a_hi)
        got_a = a1[k][T].astype(np.float64)
        assert (got_a >= a_lo - ea).all() and (got_a <= a_hi + ea).all(), (k, "a", float(np.maximum(a_lo - ea - got_a, got_a - a_hi - ea).max()))
        s = lambda g, a: lr * g / np.sqrt(a)[:, None]
        s_lo = np.minimum(s(gT - d, a_lo), s(gT - d, a_hi))
        s_hi = np.maximum(s(gT + d, a_lo), s(gT + d, a_hi))
        rel = ((ea / (2 * a_lo))[:, None] + 2.0 ** -22) * (1 + 2.0 ** -20)
        w = rel * np.maximum(np.abs(s_lo), np.abs(s_hi)) + ulp32(np.maximum(np.abs(p0[k][T]), np.abs(p1[k][T])))
        du = p1[k][T].astype(np.float64) - pT
        dp = np.maximum(du - (-s_lo + w), (-s_hi - w) - du)
        assert (dp <= 0).all(), (k, "p", float(dp.max()))
        assert (a1[k][T] > a0[k][T]).any() and (p1[k][T] != p0[k][T]).any(), k
        checked += len(T)
    return checked


def run_steps(model, E, R, D, B, n, nr, steps, use_counts=True, alpha=0.01, Dr=None, tag=""):
    Dr_ = D if Dr is None else Dr
    rng = np.random.default_rng(seed_of(model, E, R, D, B, n, nr, "rowadagrad"))
    params = oracle.init_params(oracle.MODEL_IDS[model], E, R, D, Dr_, seed=8)
    orc = oracle.Model(model, E, R, D, Dr_, margin=1.0, negative_rel=nr, params=params)
    con = engine(model, E, R, D, n, nr, alpha=alpha, params=params, Dr=Dr, use_counts=use_counts)
    assert not con.persistent_supported() and len(con._rowadagrad_acc) == len(con.trainModel.table_names)
    assert all(float(a.min()) == float(a.max()) == float(np.float32(A0)) and tuple(a.shape) == (t.shape[0],)
               for a, t in zip(con._rowadagrad_acc, con._tables))
    checked = redraws = 0
    for step in range(steps):
        orc.params = con.get_parameters()
        bh, bt, br, i = _clean_batch(model, orc, orc.params, lambda: rand_batch(rng, E, R, B, n, nr, distinct=True), B, n + nr, D, Dr_, nr)
        redraws += i
        checked += step_against_the_rule(con, orc, bh, bt, br, B, n + nr, alpha)
    assert checked > 0 and con.global_step == steps
    parity_report("row_adagrad_%s%s" % (model, tag), touched_rows_checked=checked, steps=steps, redraws=redraws, rows_excused=0)
    return con


@pytest.mark.parametrize("model,use_counts,n,nr", [("transe", True, 3, 0), ("transe", False, 2, 1), ("transh", True, 3, 0),
                                                   ("transd", True, 3, 0)])
def test_steps_follow_the_rule_on_the_oracle_gradient(model, use_counts, n, nr):
    """Three hand-fed steps at tests/test_gpu_adagrad.py's shape over all tables of the model: TransE on the sign-count path
    (reduce, then kge_transe_apply_rows_rowadagrad) and off it with a relation negative, TransH and TransD from float records
    (kge_forward_backward_rowadagrad_rows).  No gradient tables exist on any of them."""
    con = run_steps(model, 400, 40, 64, 96, n, nr, 3, use_counts=use_counts, tag="_n%d_nr%d_c%d" % (n, nr, use_counts))
    assert con._grads == []
    if model == "transe" and use_counts:
        assert con.sparse_rows and not con.sparse_inplace
    else:
        assert con.sparse_inplace and not con.sparse_rows


@pytest.mark.parametrize("model", ["transh", "transd"])
def test_steps_with_hub_copies(model):
    """R = 2, B = 256: the four relation-side rows are spread over hub copies, which hub_fold_adam_kernel adds in copy order
    before the squares are summed and the rule is applied once per row."""
    con = run_steps(model, 300, 2, 16, 256, 1, 0, 3, tag="_hub")
    assert con._grads == [] and con.sparse_inplace


def test_steps_of_transr_through_the_dense_stage():
    """TransR (De = 12, Dr = 8) keeps its dense gradient tables in one process; apply_gradients ends in
    kge_rowadagrad_update_tables -- a row of transfer_matrix is one relation's whole 96-element matrix, with ONE accumulator --
    which leaves the gradient tables zero for the next step."""
    con = run_steps("transr", 120, 9, 12, 64, 3, 0, 3, Dr=8)
    assert len(con._grads) == len(con._tables) and not con.sparse_rows and not con.sparse_inplace
    assert not any(g.any().item() for g in con._grads)
    assert tuple(con._rowadagrad_acc[2].shape) == (9,) and tuple(con._tables[2].shape) == (9, 96)


# ---- e. shared negatives --------------------------------------------------------------------------------------------------------------

class AsAdagrad(object):
    """A RowAdagrad Config as the existing shared-step modules' checks read an Adagrad one: they take the accumulators from
    `_adagrad_acc` where `_adagrad` is set and put them, with the reference's gradient, through test_gpu_adagrad.adagrad_rule_fp32
    (looked up at call time; row_rule_as_adagrads below stands in for it during the test).  Everything else, train_step included,
    is the Config's own."""

    def __init__(self, con):
        object.__setattr__(self, "_con", con)

    _adagrad = True

    @property
    def _adagrad_acc(self):
        return self._con._rowadagrad_acc

    def __getattr__(self, name):
        return getattr(self._con, name)


def row_rule_as_adagrads(p, a, g, lr):
    """adagrad_rule_fp32's signature -- p, g [n, L], (p1, a1, step) in fp32 -- with the row-wise rule and a [n]: the reference the
    shared-step modules compare a table with to 1e-5 of the step's largest move."""
    p1, a1, _, step = row_rule_fp64(p, a, g, lr)
    return p1.astype(np.float32), a1.astype(np.float32), step.astype(np.float32)


@pytest.fixture
def as_adagrad(monkeypatch):
    import test_gpu_adagrad
    monkeypatch.setattr(test_gpu_adagrad, "adagrad_rule_fp32", row_rule_as_adagrads)
    return AsAdagrad


def _one_step_of_three_tables(mod, con, names, excusable):
    """Step 0 as test_three_steps_follow_the_definition of `mod` (tests/test_gpu_shared_step.py, _grouped_step.py, _transh_step.py)
    checks each of its steps: the loss to 1e-5, rows without a record bit for bit in tables and accumulators, every other row
    within 1e-5 of the step's largest move, at most 1 % of the touched rows excused by the fp64 reference."""
    s0 = mod.state(con)
    got_loss = con.train_step()
    assert con.global_step == 1
    s1 = mod.state(con)
    res = mod.reference_step(con, s0, 0, 0.0)
    loss, want, listed, excused, near, fwd = res[:6]
    assert fwd["min_kink"] >= 1e-5, fwd["min_kink"]
    assert abs(got_loss - loss) <= 1e-5 * abs(loss)
    touched = excused_n = 0
    for i, name in enumerate(names):
        rows = listed[name]
        rest = np.setdiff1d(np.arange(len(s0[name])), rows)
        assert np.array_equal(s1[name][rest], s0[name][rest])
        acc0, acc1 = s0["a%d" % i], s1["a%d" % i]         # one per row; outside the listed rows nothing moves
        assert acc0.shape == (len(s0[name]),) and np.array_equal(acc1[rest], acc0[rest]) and (acc1[rows] > acc0[rows]).any()
        ok_rows = np.setdiff1d(rows, np.array(sorted(excused.get(name, ())), dtype=np.int64))
        touched += len(rows); excused_n += len(rows) - len(ok_rows)
        move = np.abs(want[name].astype(np.float64) - s0[name]).max()
        off = np.abs(s1[name][ok_rows].astype(np.float64) - want[name][ok_rows]).max() if len(ok_rows) else 0.0
        print("   %s: largest move %.3e, largest difference %.3e (bound %.3e)" % (name, move, off, 1e-5 * move))
        assert off <= 1e-5 * move, (name, off, move)
    assert touched > 0 and excused_n <= (0.01 * touched if excusable else 0), (excused_n, touched)


def test_a_shared_step_of_transe_by_position(as_adagrad):
    import test_gpu_shared_step as mod
    con = mod.make_config(OPT, 200, table_seed=mod.TABLE_SEEDS["Adagrad", 200])
    assert con._row_adagrad and con.sparse_rows and con.use_counts and not con.persistent_supported() and con._grads == []
    _one_step_of_three_tables(mod, as_adagrad(con), ("ent_embeddings", "rel_embeddings"), True)


def test_a_shared_step_of_transe_on_grouped_chunks(as_adagrad):
    import test_gpu_shared_grouped_step as mod
    con = mod.make_config(OPT, typed=True, table_seed=mod.TABLE_SEED)
    assert con._row_adagrad and con.sparse_rows and con.use_counts and con._grads == []
    _one_step_of_three_tables(mod, as_adagrad(con), ("ent_embeddings", "rel_embeddings"), True)


def test_a_shared_step_of_transh_on_grouped_chunks(as_adagrad):
    import test_gpu_shared_transh_step as mod
    con = mod.make_config(OPT, typed=True, table_seed=mod.TABLE_SEED)
    assert con._row_adagrad and con.sparse_inplace and not con.sparse_rows and con._grads == []
    assert con.alpha == mod.alpha_of("Adagrad")
    _one_step_of_three_tables(mod, as_adagrad(con), mod.TABLES, True)


@pytest.mark.parametrize("model", ["transd", "transr"])
def test_a_shared_step_of_transd_and_transr_on_grouped_chunks(as_adagrad, model):
    """Their modules' own measure_step / assert_step on step 0, at the rate their Adagrad runs use.  (At one rate the row-wise
    rule's largest move is at least Adagrad's -- the row's largest |g| is divided by sqrt(a + mean g^2) <= sqrt(a + g^2) -- so
    1e-5 of it is no nearer to an ulp of the tables than those modules established for Adagrad.)"""
    import importlib
    mod = importlib.import_module("test_gpu_shared_%s_step" % model)
    con = mod.make_config(OPT, typed=True, table_seed=mod.TABLE_SEEDS["Adagrad", True])
    con.set_alpha(mod.RATES["Adagrad"])
    assert con._row_adagrad and (len(con._grads) == 3) == (model == "transr") and not con.persistent_supported()
    m = mod.measure_step(as_adagrad(con), 0, "%s %s" % (model, OPT), True, con.type_constraints())
    mod.assert_step(m)
    assert m["rows"] > 0 and m["from_list"] > 0
    assert all(a.min() >= np.float32(A0) and a.max() > np.float32(A0) for a in (t.cpu().numpy() for t in con._rowadagrad_acc))


# ---- f. reproducibility -----------------------------------------------------------------------------------------------------------------

def _train_kg_small(model_name, steps):
    import openkeonspark_amd as pkg
    pkg._lib.lib().kge_set_option(b"libc_rand_restart", 1)                  # the sampler's seeds as in a new process
    con = pkg.Config()
    con.set_in_path(os.path.join(GOLDEN, "kg_small"))
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(48); con.set_nbatches(10)      # B = 600
    con.set_ent_neg_rate(3); con.set_rel_neg_rate(0); con.set_alpha(0.05); con.set_opt_method(OPT)
    con.counts_min_records = 0
    con.init()
    con.set_model_and_session(getattr(pkg, model_name))
    assert con._row_adagrad and (con.sparse_rows or con.sparse_inplace) and con._grads == []
    losses = [con.train_step() for _ in range(steps)]
    return losses, _state(con)


@pytest.mark.parametrize("model_name", ["TransH", "TransE"])
def test_training_is_reproducible_bit_for_bit(model_name):
    """Two runs from the same parameters and the same sampled batches: no sum of the step -- the sum of squares included --
    depends on scheduling, so losses, tables and accumulators agree in every bit."""
    a = _train_kg_small(model_name, 12)
    b = _train_kg_small(model_name, 12)
    assert a[0] == b[0]
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert all(np.isfinite(a[0])) and a[0][-1] < a[0][0]
    assert all(v.ndim == 1 and v.min() >= np.float32(A0) and v.max() > np.float32(A0) for v in a[1][1].values())


def test_the_dense_stage_is_reproducible_bit_for_bit():
    from test_gpu_shard_stages import _env, _ok
    torch, _lib, L = _env()
    rng = np.random.default_rng(11)
    p, a, g = rng.standard_normal((5, 40000)).astype(np.float32), (A0 + rng.random(5)).astype(np.float32), rng.standard_normal((5, 40000)).astype(np.float32)
    outs = []
    for _ in range(2):
        tp, ta, tg = (torch.from_numpy(x.copy()).cuda() for x in (p, a, g))
        one = lambda t: _lib.table_ptrs([t.data_ptr()])
        _ok(L.kge_rowadagrad_update_tables(1, one(tp), one(ta), one(tg), (ctypes.c_int64 * 4)(5), (ctypes.c_int64 * 4)(40000), 0.1, None), _lib)
        torch.cuda.synchronize()
        outs.append((tp.cpu().numpy(), ta.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and (outs[0][1] > a).all()


# ---- g. refusals ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("acc0", [0, -1])
def test_a_non_positive_initial_accumulator_is_refused(acc0):
    import openkeonspark_amd as pkg
    with pytest.raises(pkg.KgeError, match="adagrad_initial_accumulator must be positive"):
        adagrad_engine("transh", 60, 4, 16, 1, 0, acc0=acc0, opt=OPT)


def test_errors_of_the_entry_points():
    import torch
    import openkeonspark_amd as pkg
    from openkeonspark_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)

    def batch(E, R, B):
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
    con = engine("transd", 60, 4, 16, 1, 0)
    dev = batch(60, 4, 32)
    acc = [t.data_ptr() for t in con._rowadagrad_acc]
    holes = _lib.table_ptrs(acc[:2] + [None] + acc[3:])
    watched = list(con._tables) + list(con._rowadagrad_acc)
    rec, key = torch.ones((8, 16), device="cuda"), torch.arange(8, dtype=torch.int32, device="cuda")
    for ptrs in (holes, None):
        refused(lambda: L.kge_forward_backward_rowadagrad_rows(
            ctypes.byref(con._desc), con._tab_ptrs, ptrs, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 32, 1, 32, 32, 0.01,
            con._loss.data_ptr(), con._stream()), KGE_ERR_BAD_ARG, watched)
        refused(lambda: L.kge_float_records_apply_rowadagrad(
            ctypes.byref(con._desc), con._tab_ptrs, ptrs, rec.data_ptr(), key.data_ptr(), 8, 32, 1, 0.01, con._stream()),
            KGE_ERR_BAD_ARG, watched)
    grads = [torch.ones_like(t) for t in con._tables]
    g_ptrs = _lib.table_ptrs([g.data_ptr() for g in grads])
    rows_ = (ctypes.c_int64 * 4)(*[t.shape[0] for t in con._tables])
    lens_ = (ctypes.c_int64 * 4)(*[t.shape[1] for t in con._tables])
    for ptrs in (holes, None):
        refused(lambda: L.kge_rowadagrad_update_tables(4, con._tab_ptrs, ptrs, g_ptrs, rows_, lens_, 0.01, con._stream()),
                KGE_ERR_BAD_ARG, watched + grads)
    for bad_rows, bad_lens in (((ctypes.c_int64 * 4)(60, -1, 4, 60), lens_), (rows_, (ctypes.c_int64 * 4)(16, 0, 16, 16)),
                               (rows_, (ctypes.c_int64 * 4)(16, 16, (1 << 24) + 1, 16))):
        refused(lambda: L.kge_rowadagrad_update_tables(4, con._tab_ptrs, con._rowadagrad_ptrs, g_ptrs, bad_rows, bad_lens, 0.01, con._stream()),
                KGE_ERR_BAD_ARG, watched + grads)
    refused(lambda: L.kge_rowadagrad_update_tables(5, con._tab_ptrs, con._rowadagrad_ptrs, g_ptrs, rows_, lens_, 0.01, con._stream()),
            KGE_ERR_BAD_ARG, watched + grads)
    cte = engine("transe", 60, 4, 16, 1, 0)
    rows, counts, n1 = (torch.zeros(4, dtype=torch.int32, device="cuda"), torch.ones((4, 16), dtype=torch.int32, device="cuda"),
                        torch.ones(1, dtype=torch.int32, device="cuda"))
    for a_ent, a_rel in ((cte._rowadagrad_acc[0].data_ptr(), None), (None, cte._rowadagrad_acc[1].data_ptr())):
        refused(lambda: L.kge_transe_apply_rows_rowadagrad(
            ctypes.byref(cte._desc), cte._tables[0].data_ptr(), cte._tables[1].data_ptr(), a_ent, a_rel, rows.data_ptr(), counts.data_ptr(),
            n1.data_ptr(), 4, 32, 0.01, cte._stream()), KGE_ERR_BAD_ARG, list(cte._tables) + list(cte._rowadagrad_acc))
    # TransR has no record path: the row entry points say so, the tables stay
    ctr = engine("transr", 60, 4, 16, 1, 0, Dr=8)
    dev = batch(60, 4, 32)
    watched = list(ctr._tables) + list(ctr._rowadagrad_acc)
    refused(lambda: L.kge_forward_backward_rowadagrad_rows(
        ctypes.byref(ctr._desc), ctr._tab_ptrs, ctr._rowadagrad_ptrs, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 32, 1, 32, 32,
        0.01, ctr._loss.data_ptr(), ctr._stream()), KGE_ERR_UNSUPPORTED, watched)
    refused(lambda: L.kge_float_records_apply_rowadagrad(
        ctypes.byref(ctr._desc), ctr._tab_ptrs, ctr._rowadagrad_ptrs, rec.data_ptr(), key.data_ptr(), 8, 32, 1, 0.01, ctr._stream()),
        KGE_ERR_UNSUPPORTED, watched)
    # no persistent launch, on any path
    for c in (con, cte, ctr):
        assert not c.persistent_supported()
        with pytest.raises(pkg.KgeError, match="persistent"):
            c.train_steps(2, persistent=True)
    small = engine("transe", 60, 4, 16, 1, 0, use_counts=False)
    assert small.sparse_inplace and not small.persistent_supported()
    # the optimizers beside it keep their refusals
    with pytest.raises(pkg.KgeError, match="TransR"):
        adagrad_engine("transr", 60, 4, 16, 1, 0, Dr=8, opt="LazyAdam")
