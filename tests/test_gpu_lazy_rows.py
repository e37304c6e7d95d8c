"""opt_method "LazyAdam" from float gradient records: TransH, TransD and TransE off the sign-count path
(kge_forward_backward_adam_rows / kge_float_records_apply_adam, csrc/transe_counts.hip segsum_adam_runs_kernel +
hub_fold_adam_kernel).  Opt-in and NON-PARITY: the reference trains with TF1's AdamOptimizer, which moves every row of every
table each step (distribute_training.py:95-101); the lazy rule applies the same element formula to the rows a step has a record
for -- their moments included -- and leaves every other row alone.

Checked here in one process: the stage alone against the rule written out in fp32 numpy (moments bit for bit: the order of
every sum is fixed; values to the accuracy of the hardware square root), whole steps against the rule on the CPU oracle's
gradient, the hub copies, odd widths, the errors, and run-to-run reproducibility.  Ranks and the driver: tests/test_gpu_lazy_rows_dp.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity_report
from oracle import oracle
from test_gpu_models import make_engine, rand_batch, seed_of

pytestmark = pytest.mark.gpu

RTOL = 1e-5              # BASELINE's parity bar on the gradient (tests/test_gpu_models.py RTOL)
B1, B2, EPS = 0.9, 0.999, 1e-8
ENT_SIDE = ("ent_embeddings", "ent_transfer")       # indexed by h and t; every other table by r
PKG_NAMES = {"transe": "TransE", "transh": "TransH", "transd": "TransD", "transr": "TransR"}


def clean_batch(model, orc, p0, make, B, N, D, nr, tries=40):
    """A batch free of hinge ties (batch_without_ties' criterion, 1e-4) AND of elements of h^ + r^ - t^ within 1e-6 of zero
    (torch_ref.near_kink_rows), drawn again until both hold: no row is excused afterwards.  -> (bh, bt, br, redraws)."""
    from torch_ref import near_kink_rows
    for i in range(tries):
        bh, bt, br = make()
        if np.abs(orc.hinge_margins(bh, bt, br, B, N)).min() <= 1e-4:
            continue
        if near_kink_rows(model, p0, bh, bt, br, B, N, D, D, tol=1e-6, negative_rel=nr)[1] == 0:
            return bh, bt, br, i
    raise AssertionError("no batch without ties and near-zero elements in %d draws" % tries)


def state_of(con):
    names = con.trainModel.table_names
    return (con.get_parameters(), {k: con._adam_m[i].cpu().numpy() for i, k in enumerate(names)},
            {k: con._adam_v[i].cpu().numpy() for i, k in enumerate(names)})


def touched_rows(names, active, bh, bt, br, B):
    """{table: sorted rows}: for every group with an active hinge, the h, t, r of its positive and of its ACTIVE negatives."""
    bh, bt, br = (np.asarray(x) for x in (bh, bt, br))
    ent, rel = set(), set()
    for b in np.nonzero(active.any(1))[0]:
        idx = [b] + [b + B * (k + 1) for k in np.nonzero(active[b])[0]]
        ent |= set(bh[idx].tolist()) | set(bt[idx].tolist())
        rel |= set(br[idx].tolist())
    return {k: np.array(sorted(ent if k in ENT_SIDE else rel), dtype=np.int64) for k in names}


def lazy_step_against_the_rule(model, con, orc, bh, bt, br, B, N, t, alpha):
    """One hand-fed step of `con` against the lazy rule on the oracle's gradient, from the state both start from.
    -> number of touched rows checked (over all tables)."""
    from parity_util import _f32_constants, adam_step_fp64, adam_update_explained
    names = con.trainModel.table_names
    p0, m0, v0 = state_of(con)
    orc.params = {k: v.copy() for k, v in p0.items()}
    active = orc.hinge_margins(bh, bt, br, B, N) > 0           # [B, N]
    loss_o, g_o = orc.grad(bh, bt, br, B, N)
    touched = touched_rows(names, active, bh, bt, br, B)
    loss_g = con.train_step(bh, bt, br, None)
    assert abs(loss_g - loss_o) <= 2e-5 * abs(loss_o), (loss_g, loss_o)
    p1, m1, v1 = state_of(con)
    lr_t = float(oracle.adam_lr_t(alpha, B1, B2, t))
    b1f, b2f, omb1, omb2, _ = _f32_constants(B1, B2, EPS)
    checked = 0
    for k in names:
        T = touched[k]
        rest = np.setdiff1d(np.arange(p0[k].shape[0]), T)
        # rows without a record: nothing moves, not even the moments
        np.testing.assert_array_equal(p1[k][rest], p0[k][rest], err_msg=k)
        np.testing.assert_array_equal(m1[k][rest], m0[k][rest], err_msg=k)
        np.testing.assert_array_equal(v1[k][rest], v0[k][rest], err_msg=k)
        assert (g_o[k][rest] == 0).all(), k
        if not len(T):
            continue
        # rows with a record: the element rule on the oracle's gradient, zero-gradient elements included; no row skipped
        pT, mT, vT, gT = (a[T].astype(np.float64) for a in (p0[k], m0[k], v0[k], g_o[k]))
        du_o = adam_step_fp64(pT, mT, vT, gT, lr_t, B1, B2, EPS)
        rep = adam_update_explained(p0[k][T], m0[k][T], v0[k][T], g_o[k][T], p1[k][T].astype(np.float64) - p0[k][T], du_o, lr_t)
        D = p0[k].shape[1]
        assert rep["unexplained"].size == 0, (t, k, [(int(T[j // D]), int(j % D)) for j in rep["unexplained"][:8]])
        # the moments: what a gradient within d of the oracle's makes of them, plus two fp32 ulps of the result
        d = RTOL * np.abs(g_o[k]).max()
        m_exp = b1f * mT + omb1 * gT
        v_exp = b2f * vT + omb2 * gT * gT
        ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
        dm = np.abs(m1[k][T] - m_exp) - (omb1 * d + 2 * ulp(m_exp))
        dv = np.abs(v1[k][T] - v_exp) - (omb2 * (2 * np.abs(gT) * d + d * d) + 2 * ulp(v_exp))
        assert (dm <= 0).all(), (t, k, "m", float(dm.max()))
        assert (dv <= 0).all(), (t, k, "v", float(dv.max()))
        checked += len(T)
    return checked


def run_steps(model, E, R, D, B, n, nr, steps, use_counts=True, alpha=0.01, seed=8, tag=""):
    rng = np.random.default_rng(seed_of(model, E, R, D, B, n, nr, "lazy-rows"))
    params = oracle.init_params(oracle.MODEL_IDS[model], E, R, D, D, seed=seed)
    orc = oracle.Model(model, E, R, D, D, margin=1.0, negative_rel=nr, params=params)
    con = make_engine(model, E, R, D, n, nr, margin=1.0, opt="LazyAdam", alpha=alpha, params=params, use_counts=use_counts)
    assert con._lazy_adam and con.sparse_inplace and not con.sparse_rows and not con._adam and con._grads == []
    assert len(con._adam_m) == len(con._adam_v) == len(con.trainModel.table_names)
    assert not con.persistent_supported()
    checked = redraws = 0
    for step in range(steps):
        orc.params = con.get_parameters()
        bh, bt, br, i = clean_batch(model, orc, orc.params, lambda: rand_batch(rng, E, R, B, n, nr, distinct=True), B, n + nr, D, nr)
        redraws += i
        checked += lazy_step_against_the_rule(model, con, orc, bh, bt, br, B, n + nr, step + 1, alpha)
    assert checked > 0 and con.global_step == steps
    parity_report("lazy_rows_%s%s" % (model, tag), touched_rows_checked=checked, steps=steps, redraws=redraws, rows_excused=0)
    return con, orc, rng


@pytest.mark.parametrize("model,use_counts,n,nr", [("transh", True, 3, 0), ("transd", True, 3, 0), ("transe", False, 3, 0),
                                                   ("transe", False, 2, 1)])
def test_lazy_adam_from_float_records_follows_the_rule(model, use_counts, n, nr):
    """Four hand-fed steps over ALL tables of the model (test_lazy_adam_moves_the_touched_rows_only's construction).  The case
    with a relation negative is TransE's: for a projecting model such a negative changes both projected entities, is no
    single-slot corruption and is refused by the in-place step (test_errors_of_the_lazy_rows_path)."""
    run_steps(model, 400, 40, 64, 96, n, nr, 4, use_counts=use_counts, tag="_n%d_nr%d" % (n, nr))


@pytest.mark.parametrize("model", ["transh", "transd"])
def test_lazy_adam_with_hub_copies(model):
    """R = 2, B = 256: record_space spreads the four relation-side rows over hub_k = 2 * 256 / (64 * 4) = 2 copies, which
    hub_fold_adam_kernel adds in copy order before the rule is applied per row.  Then one step in which relation 1 takes no
    record at all: its rows and moments in every relation-side table keep their bits -- the per-row mark decides, not the sum."""
    E, R, D, B, n = 300, 2, 16, 256, 1
    con, orc, rng = run_steps(model, E, R, D, B, n, 0, 4, tag="_hub")
    names = con.trainModel.table_names

    def only_relation_0():
        bh, bt, br = rand_batch(rng, E, R, B, n, 0, distinct=True)
        return bh, bt, np.zeros_like(br)
    orc.params = con.get_parameters()
    bh, bt, br, _ = clean_batch(model, orc, orc.params, only_relation_0, B, n, D, 0)
    p0, m0, v0 = state_of(con)
    assert all(np.abs(m0[k][1]).max() > 0 for k in names if k not in ENT_SIDE)      # relation 1 has moments to lose
    lazy_step_against_the_rule(model, con, orc, bh, bt, br, B, n, 5, 0.01)
    p1, m1, v1 = state_of(con)
    for k in names:
        if k in ENT_SIDE:
            continue
        for a0, a1 in ((p0, p1), (m0, m1), (v0, v1)):
            np.testing.assert_array_equal(a1[k][1], a0[k][1], err_msg=k)
            assert (a1[k][0] != a0[k][0]).any(), k


@pytest.mark.parametrize("D", [7, 50, 100])
def test_lazy_adam_at_odd_widths(D):
    """Widths that are no multiple of 4 (scalar loads and stores) nor of the team width: one step against the rule."""
    run_steps("transh", 120, 5, D, 64, 2, 0, 1, tag="_D%d" % D)


def test_errors_of_the_lazy_rows_path():
    import torch
    import openkeonspark_amd as pkg
    from openkeonspark_amd import _lib
    L = _lib.lib()
    # TransR has no record path: the entry point says so and leaves the tables alone, Config refuses the combination
    con = make_engine("transr", 60, 4, 16, 1, 0, Dr=8)
    before = [t.clone() for t in con._tables]
    zeros = [torch.zeros_like(t) for t in con._tables]
    ptrs = _lib.table_ptrs([z.data_ptr() for z in zeros])
    bh, bt, br = rand_batch(np.random.default_rng(1), 60, 4, 32, 1, 0, distinct=True)
    dev = torch.from_numpy(np.stack([bh, bt, br]).astype(np.int32)).cuda()
    rc = L.kge_forward_backward_adam_rows(ctypes.byref(con._desc), con._tab_ptrs, ptrs, ptrs, dev[0].data_ptr(), dev[1].data_ptr(),
                                          dev[2].data_ptr(), 32, 1, 32, 32, 0.01, B1, B2, EPS, con._loss.data_ptr(), con._stream())
    torch.cuda.synchronize()
    assert rc == -4                                            # KGE_ERR_UNSUPPORTED (include/kge_mi355.h)
    L.kge_clear_error()
    for t, b, z in zip(con._tables, before, zeros):
        assert torch.equal(t, b) and not z.any().item()
    with pytest.raises(pkg.KgeError, match="TransR"):
        make_engine("transr", 60, 4, 16, 1, 0, Dr=8, opt="LazyAdam")
    # negatives that are not single-slot corruptions are left out and counted: the step raises, as the SGD form does
    rng = np.random.default_rng(2)
    for model, nr in (("transh", 0), ("transh", 1)):
        con = make_engine(model, 300, 7, 64, 3, nr, opt="LazyAdam")
        bh, bt, br = rand_batch(rng, 300, 7, 160, 3, nr, foreign=0.3 if nr == 0 else 0.0, distinct=True)
        with pytest.raises(pkg.KgeError, match="single-slot"):
            con.train_step(bh, bt, br, None)


def adam_rule_fp32(p, m, v, g, lr_t):
    """adam_one (csrc/optim_dev.hpp) in numpy fp32: every product, sum, root and quotient rounded once, in its order.
    -> (p1, m1, v1, step): m1 and v1 are sums and products only and are what the device must hold bit for bit; `step` is
    lr_t m1 / (sqrt(v1) + eps), whose root the device takes with v_sqrt_f32 (__fsqrt_rn without OCML_BASIC_ROUNDED_OPERATIONS is
    the native root: within one ulp, not correctly rounded), so p1 is compared through p_allowance."""
    f = np.float32
    b1, b2, eps, lr_t = f(B1), f(B2), f(EPS), f(lr_t)
    mi, vi = m * b1, v * b2
    nz = g != 0
    mi = np.where(nz, mi + g * (f(1) - b1), mi).astype(f)
    vi = np.where(nz, vi + (g * g).astype(f) * (f(1) - b2), vi).astype(f)
    step = ((lr_t * mi) / (np.sqrt(vi) + eps)).astype(f)
    return (p - step).astype(f), mi, vi, step


def p_allowance(p1, step):
    """How far the device's p1 may lie from adam_rule_fp32's: a root within one ulp moves the denominator sqrt(v) + eps by at
    most two of its ulps (the root's, and the rounding of the sum landing one further), i.e. by 2^-22 relative; the rounded
    quotient then moves by at most 2^-22 |step| plus one of its own ulps (2^-23 |step|), together under 2^-21 |step|; and the
    rounded difference p - step by that plus one ulp of the result."""
    return 2.0 ** -21 * np.abs(step).astype(np.float64) + np.spacing(np.abs(p1)).astype(np.float64)


@pytest.mark.parametrize("model,D", [("transd", 4), ("transd", 7), ("transd", 200), ("transh", 1024), ("transe", 50),
                                     # the other rungs: float4 (16, 2) and (32, 4); scalar (16, 2), (32, 4), (64, 4), (64, 8), (64, 16)
                                     ("transd", 100), ("transh", 260), ("transe", 30), ("transh", 70), ("transd", 130), ("transe", 258),
                                     ("transh", 514)])
def test_the_apply_stage_alone_bit_for_bit(model, D):
    """kge_float_records_apply_adam on made-up records, keys over the whole virtual row space (entity rows, ent_transfer rows,
    hub copies of both relation-side tables) plus keys that carry no record (-1, -7, rows, rows + 5): m and v must equal,
    BIT FOR BIT, the rule in fp32 numpy on per-row sums taken in record order and hub copies added in copy order (any other
    order or a partial sum shows there), p within what the device's square root allows (p_allowance) -- and rows without a
    record keep every bit of all three.  Twice in a row: the marks and copy sums the first call leaves must be clean."""
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    E, R, n_pos_total, n_neg, M = 50, 3, 1000, 1, 3000
    con = make_engine(model, E, R, D, n_neg, 0)
    names = con.trainModel.table_names
    ent_rows = (2 if model == "transd" else 1) * E
    hub_rows = (1 if model == "transe" else 2) * R
    hub_k = max(1, ((1 if model == "transe" else 2) * n_pos_total) // (hub_rows * 64))
    assert hub_k >= 2
    rows = ent_rows + hub_k * hub_rows
    rng = np.random.default_rng(seed_of(model, D, "stage"))
    shapes = [tuple(t.shape) for t in con._tables]
    P = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    Mm = [(0.1 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    V = [(0.01 * rng.random(s)).astype(np.float32) for s in shapes]
    dev = lambda arrs: [torch.from_numpy(a.copy()).cuda() for a in arrs]
    tp, tm, tv = dev(P), dev(Mm), dev(V)
    for call in range(2):
        rec = rng.standard_normal((M, D)).astype(np.float32)
        rec[rng.random((M, D)) < 0.2] = 0.0
        rec[M // 2] = 0.0                                                  # a record of zeros still touches its row
        keys = rng.integers(0, rows, M).astype(np.int32)
        keys[rng.random(M) < 0.5] = rng.integers(ent_rows, rows)            # one hot hub copy: a long run
        keys[rng.random(M) < 0.1] = -1
        keys[:4] = (-7, rows, rows + 5, 2 ** 31 - 1)
        spared = rng.integers(0, rows, 8)                                   # some rows surely without a record
        keys[np.isin(keys, spared)] = -1
        lr_t = 0.01 * (call + 1)
        # expectation
        valid = (keys >= 0) & (keys < rows)
        sums, seen = {}, set()
        for i in np.nonzero(valid)[0]:                                      # record order within a key
            k = int(keys[i])
            sums[k] = rec[i].copy() if k not in sums else (sums[k] + rec[i]).astype(np.float32)
        want = [[a.copy() for a in X] for X in (P, Mm, V)]
        slack = [np.zeros(a.shape, np.float64) for a in P]                 # rows without a record: every bit

        def apply(t, r, g):
            want[0][t][r], want[1][t][r], want[2][t][r], step = adam_rule_fp32(P[t][r], Mm[t][r], V[t][r], g, lr_t)
            slack[t][r] = p_allowance(want[0][t][r], step)
            seen.add((t, r))
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
        assert len(seen) < sum(s[0] for s in shapes)
        d_rec, d_key = torch.from_numpy(rec).cuda(), torch.from_numpy(keys).cuda()
        _lib.check(L.kge_float_records_apply_adam(
            ctypes.byref(con._desc), _lib.table_ptrs([t.data_ptr() for t in tp]), _lib.table_ptrs([t.data_ptr() for t in tm]),
            _lib.table_ptrs([t.data_ptr() for t in tv]), d_rec.data_ptr(), d_key.data_ptr(), M, n_pos_total, n_neg, lr_t, B1, B2, EPS,
            con._stream()), L)
        torch.cuda.synchronize()
        for X, tX, what in ((want[1], tm, "m"), (want[2], tv, "v")):
            for t, name in enumerate(names):
                np.testing.assert_array_equal(tX[t].cpu().numpy(), X[t], err_msg="%s of %s, call %d" % (what, name, call))
        got_p = [t.cpu().numpy() for t in tp]
        for t, name in enumerate(names):
            off = np.abs(got_p[t].astype(np.float64) - want[0][t])
            assert (off <= slack[t]).all(), ("p of %s, call %d" % (name, call), float((off - slack[t]).max()))
            untouched = slack[t].max(axis=1) == 0
            np.testing.assert_array_equal(got_p[t][untouched], P[t][untouched], err_msg="untouched p of %s, call %d" % (name, call))
        P, Mm, V = got_p, want[1], want[2]                                  # the next call starts from the device's state


def _train_kg_small(model_name, steps):
    import openkeonspark_amd as pkg
    pkg._lib.lib().kge_set_option(b"libc_rand_restart", 1)                  # the sampler's seeds as in a new process
    con = pkg.Config()
    con.set_in_path(os.path.join(GOLDEN, "kg_small"))
    con.set_work_threads(8); con.set_bern(1); con.set_dimension(48); con.set_nbatches(10)      # B = 600
    con.set_ent_neg_rate(3); con.set_rel_neg_rate(0); con.set_alpha(0.02); con.set_opt_method("LazyAdam")
    con.init()
    con.set_model_and_session(getattr(pkg, model_name))
    assert con.sparse_inplace and con._lazy_adam
    losses = [con.train_step() for _ in range(steps)]
    return losses, state_of(con), (con._beta1_power, con._beta2_power)


@pytest.mark.parametrize("model_name", ["TransH", "TransD"])
def test_lazy_rows_training_is_reproducible_bit_for_bit(model_name):
    """Two runs from the same parameters and the same sampled batches: no sum of the step depends on scheduling, so losses,
    tables and moments agree in every bit -- and the run trains."""
    a = _train_kg_small(model_name, 20)
    b = _train_kg_small(model_name, 20)
    assert a[0] == b[0] and a[2] == b[2]
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert all(np.isfinite(a[0])) and np.mean(a[0][-5:]) < np.mean(a[0][:5])
