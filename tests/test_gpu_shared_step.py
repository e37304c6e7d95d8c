"""Training on shared negatives through Config.train_step (Config.set_shared_negatives; NON-PARITY, opt-in).

Every step is compared with a torch fp64 reference of the defined loss on the EXPANDED batch -- negative k of positive b spelled
out as (h_b, c_k, r_b) or (c_k, t_b, r_b), tests/torch_ref.py loss_and_grads.  That function has no weights, so a masked pair is
spelled as the positive itself: its hinge is max(p - p + margin, 0) = margin with a gradient of exactly zero, and the constant
n_masked * margin / denom is taken off the loss.  The gradient goes through the test modules' fp32 restatements of the optimizer
rules (SGD here, tests/test_gpu_lazy_rows.py adam_rule_fp32, tests/test_gpu_adagrad.py adagrad_rule_fp32) on the rows the
definition lists, and a table may differ from the result by 1e-5 of the step's largest move (tests/test_gpu_sparse.py's bound on
the sparse step), except in rows torch_ref.near_kink_rows excuses; the fp64 reference alone may excuse at most 1 % of the touched
rows.  LazyAdam runs at adam_epsilon = 1e-4 (ADAM_EPS below has the reasoning and the figures measured at the default 1e-8,
where Adam's first-step quotient amplifies fp32 gradient rounding beyond that bound).  Then: two runs are bit-identical, a resumed run repeats the interrupted one bit for bit, and a Config that never mentions
the feature is untouched by it."""
import os

import numpy as np
import pytest

import shared_neg_ref as ref
from conftest import parity_report

pytestmark = pytest.mark.gpu

E, R, MARGIN, ALPHA = 300, 6, 1.0, 0.05
P, N, SEED = 16, 4, 12345
# initialisation seeds of the runs compared with the fp64 reference: chosen so that the reference finds (almost) no element of
# h^ + r^ - t^ within 1e-6 of zero in the three steps (at width 200 a step scores 96 x 5 x 200 elements, and one such element
# excuses the seven rows of its group)
TABLE_SEEDS = {("SGD", 200): 13, ("LazyAdam", 200): 23, ("Adagrad", 200): 13}
# LazyAdam's epsilon in these runs.  The first Adam steps move an element by about alpha g / (|g| + eps'), eps' = eps /
# sqrt(1 - beta2) = 32 eps: the fp32 rounding dg of a gradient element reaches the table multiplied by up to alpha / eps'.  The
# gradient elements are sums of terms of about 3e-2 / |row|, so dg is about 1e-10, and at TF1's default eps = 1e-8 an element
# whose gradient nearly cancels is off by up to alpha * 1e-10 / 3.2e-7 = 3e-4 alpha, thirty times the bound of 1e-5 of the
# largest move (alpha) that holds here: no fp32 gradient can meet it, whatever its order of operations (measured at the default:
# 1 to 8 of 30 000 elements per step beyond the bound, the largest 2.3e-5 against 5.0e-7).  At eps = 1e-4 the factor is
# alpha / 3.2e-3 and the same rounding stays four hundred times inside the bound, so the comparison tests the step and not the
# conditioning of Adam's quotient.
ADAM_EPS = 1e-4


def graph():
    rng = np.random.default_rng(5)
    n = 960
    h = rng.integers(0, E, n); r = rng.integers(0, R, n)
    t = (h + 1 + rng.integers(0, E - 1, n)) % E
    return h.astype(np.int64), t.astype(np.int64), r.astype(np.int64)


def make_config(opt, D, shared=True, mention=True, table_seed=3):
    import torch
    import openkeonspark_amd as ok
    con = ok.Config()
    con.set_work_threads(4); con.set_bern(1); con.set_dimension(D); con.set_ent_neg_rate(N); con.set_rel_neg_rate(0)
    con.set_alpha(ALPHA); con.set_margin(MARGIN); con.set_opt_method(opt); con.set_nbatches(10)
    con.sparse_rows = True
    con.seed = table_seed
    con.adam_epsilon = ADAM_EPS
    if shared:
        con.set_shared_negatives(P, seed=SEED)
    elif mention:
        con.set_shared_negatives(0)
    con.lib.kge_set_option(b"libc_rand_restart", 1)
    con.init_from_arrays(E, R, *graph())
    con.set_model_and_session(ok.TransE)
    return con


def state(con):
    s = {k: v.copy() for k, v in con.get_parameters().items()}
    if con._lazy_adam:
        s.update({"m%d" % i: t.cpu().numpy() for i, t in enumerate(con._adam_m)})
        s.update({"v%d" % i: t.cpu().numpy() for i, t in enumerate(con._adam_v)})
    if con._adagrad:
        s.update({"a%d" % i: t.cpu().numpy() for i, t in enumerate(con._adagrad_acc)})
    return s


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def reference_step(con, s0, step, lr_t):
    """The tables (and slots) the definition gives from state s0 for the step `con` has just trained; also what is excused."""
    from torch_ref import loss_and_grads, near_kink_rows
    from test_gpu_adagrad import adagrad_rule_fp32
    import test_gpu_lazy_rows
    from test_gpu_lazy_rows import adam_rule_fp32
    D, B = con.hidden_size, con.batch_size
    cand, pair = con.shared_negatives_of(step)
    pos = con._sparse_buf["shared_batch"].cpu().numpy()[:, :B].astype(np.int64)
    h, t, r = pos
    params = {"ent_embeddings": s0["ent_embeddings"], "rel_embeddings": s0["rel_embeddings"]}
    denom = B * N
    want = ref.forward(params["ent_embeddings"], params["rel_embeddings"], h, t, r, cand, pair, P, MARGIN, denom)
    bh, bt, br = ref.expand(h, t, r, cand, pair, P, B)
    masked = (pair & 2) != 0
    for k in range(N):      # a masked pair: the positive itself (zero gradient, hinge = margin)
        o = (k + 1) * B
        bh[o:o + B][masked[:, k]] = h[masked[:, k]]; bt[o:o + B][masked[:, k]] = t[masked[:, k]]
    loss, g = loss_and_grads("transe", params, bh, bt, br, B, N, MARGIN, D, D)
    loss -= masked.sum() * MARGIN / denom
    assert abs(loss - want["loss"]) <= 1e-9 * max(abs(loss), 1e-9)      # (the two restatements of the definition agree)
    keys = want["keys"]
    listed = {"ent_embeddings": np.unique(keys[(keys >= 0) & (keys < E)]), "rel_embeddings": np.unique(keys[keys >= E]) - E}
    out = {}
    for i, name in enumerate(("ent_embeddings", "rel_embeddings")):
        p0, gi, rows = s0[name], g[name].astype(np.float32), listed[name]
        assert not np.abs(g[name][np.setdiff1d(np.arange(len(p0)), rows)]).any()      # no gradient outside the listed rows
        p1 = p0.copy()
        if con._lazy_adam:
            m1, v1 = s0["m%d" % i].copy(), s0["v%d" % i].copy()
            eps0, test_gpu_lazy_rows.EPS = test_gpu_lazy_rows.EPS, ADAM_EPS      # (the restatement reads its module's constant)
            try:
                p1[rows], m1[rows], v1[rows], _ = adam_rule_fp32(p0[rows], m1[rows], v1[rows], gi[rows], lr_t)
            finally:
                test_gpu_lazy_rows.EPS = eps0
            out["m%d" % i], out["v%d" % i] = m1, v1
        elif con._adagrad:
            a1 = s0["a%d" % i].copy()
            p1[rows], a1[rows], _ = adagrad_rule_fp32(p0[rows], a1[rows], gi[rows], ALPHA)
            out["a%d" % i] = a1
        else:
            p1 = (p0 - np.float32(ALPHA) * gi).astype(np.float32)
        out[name] = p1
    excused, near = near_kink_rows("transe", params, bh, bt, br, B, N, D, D, tol=1e-6)
    return loss, out, listed, excused, near, want


@pytest.mark.parametrize("D", [32, 200])
@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_three_steps_follow_the_definition(opt, D):
    con = make_config(opt, D, table_seed=TABLE_SEEDS.get((opt, D), 3))
    assert con.sparse_rows and con.use_counts and not con.persistent_supported() and con._grads == []
    touched = excused_n = 0
    for step in range(3):
        s0 = state(con)
        lr_t = float(con._adam_lr_t()) if con._lazy_adam else 0.0
        got_loss = con.train_step()
        assert con.global_step == step + 1
        s1 = state(con)
        loss, want, listed, excused, near, fwd = reference_step(con, s0, step, lr_t)
        assert fwd["min_kink"] >= 1e-5, fwd["min_kink"]      # no hinge within rounding of its kink on these seeds
        print("%s D %d step %d: loss %.7f (fp64 %.7f), listed rows %d + %d, near-zero elements %d, min kink %.2e"
              % (opt, D, step, got_loss, loss, len(listed["ent_embeddings"]), len(listed["rel_embeddings"]), near, fwd["min_kink"]))
        assert abs(got_loss - loss) <= 1e-5 * abs(loss)
        for name in ("ent_embeddings", "rel_embeddings"):
            rows = listed[name]
            rest = np.setdiff1d(np.arange(len(s0[name])), rows)
            assert np.array_equal(s1[name][rest], s0[name][rest])             # a row without a record keeps every bit
            ok_rows = np.setdiff1d(rows, np.array(sorted(excused[name]), dtype=np.int64))
            touched += len(rows); excused_n += len(rows) - len(ok_rows)
            move = np.abs(want[name].astype(np.float64) - s0[name]).max()
            off = np.abs(s1[name][ok_rows].astype(np.float64) - want[name][ok_rows]).max() if len(ok_rows) else 0.0
            print("   %s: largest move %.3e, largest difference %.3e (bound %.3e)" % (name, move, off, 1e-5 * move))
            assert off <= 1e-5 * move, (name, off, move)
        for k in want:
            if k[0] in "mva" and k[1:].isdigit():      # slots: outside the listed rows nothing moves
                i = int(k[1:])
                rest = np.setdiff1d(np.arange(len(s0[k])), listed[("ent_embeddings", "rel_embeddings")[i]])
                assert np.array_equal(s1[k][rest], s0[k][rest])
    parity_report("shared_step_%s_D%d" % (opt, D), touched_rows=touched, rows_excused=excused_n)
    assert excused_n <= 0.01 * touched, (excused_n, touched)


@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_reproducible_and_resumable_bit_for_bit(opt, tmp_path):
    from openkeonspark_amd import distribute_training as dt
    import openkeonspark_amd as ok
    a = make_config(opt, 32)
    la = [a.train_step() for _ in range(2)]
    dt.save_checkpoint(a, str(tmp_path))
    la.append(a.train_step())
    b = make_config(opt, 32)
    lb = [b.train_step() for _ in range(3)]
    assert la == lb and same_bits(state(a), state(b))
    # resumed after step 2: step 3 repeats the interrupted run's
    c = make_config(opt, 32, table_seed=4)
    assert dt.restore_checkpoint(c, os.path.join(str(tmp_path), "model.ckpt-2.npz")) == 2
    assert c.train_step() == la[2] and same_bits(state(a), state(c))
    # another chunk, another seed, or the option off: refused
    for kw in (dict(chunk=8, seed=SEED), dict(chunk=P, seed=SEED + 1), dict(chunk=0, seed=0)):
        d = ok.Config()
        d.set_work_threads(4); d.set_dimension(32); d.set_ent_neg_rate(N); d.set_opt_method(opt); d.set_nbatches(10)
        d.sparse_rows = True
        d.set_shared_negatives(kw["chunk"], seed=kw["seed"])
        d.init_from_arrays(E, R, *graph())
        d.set_model_and_session(ok.TransE)
        with pytest.raises(ok.KgeError, match="shared negatives"):
            dt.restore_checkpoint(d, os.path.join(str(tmp_path), "model.ckpt-2.npz"))


@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_option_off_is_the_step_as_it_was(opt):
    """set_shared_negatives(0) against a Config that never mentions the feature: the same losses and tables, bit for bit."""
    a = make_config(opt, 32, shared=False, mention=True)
    la = [a.train_step() for _ in range(2)]
    b = make_config(opt, 32, shared=False, mention=False)      # (one engine per process: a Config trains before the next one is made)
    lb = [b.train_step() for _ in range(2)]
    assert la == lb and same_bits(state(a), state(b))
    assert a._sparse_buf is not None and "cand" not in a._sparse_buf


def test_refusals_of_a_configured_model():
    import openkeonspark_amd as ok
    con = make_config("SGD", 32)
    with pytest.raises(ok.KgeError, match="before set_model_and_session"):
        con.set_shared_negatives(8)
    with pytest.raises(ok.KgeError, match="hand-fed"):
        con.train_step(np.zeros(5 * (1 + N)), np.ones(5 * (1 + N)), np.zeros(5 * (1 + N)), None)
    with pytest.raises(ok.KgeError, match="shared negatives"):
        con.train_steps(2, persistent=True)
    assert len(con.train_steps(2)) == 2 and con.global_step == 2
    con.prefetch_sampling = True          # ignored: nothing is drawn ahead
    con.train_step()
    assert con._prefetched is None
    con.force_data_parallel = True        # more than one rank (here: the one-rank rehearsal of the exchange)
    with pytest.raises(ok.KgeError, match="one rank"):
        con.train_step()
    for opt, words in (("Adam", "dense count image"),):
        bad = ok.Config()
        bad.set_work_threads(4); bad.set_dimension(32); bad.set_ent_neg_rate(N); bad.set_opt_method(opt); bad.set_nbatches(10)
        bad.set_shared_negatives(P)
        bad.init_from_arrays(E, R, *graph())
        with pytest.raises(ok.KgeError, match=words):
            bad.set_model_and_session(ok.TransE)
    for model in ("TransH", "TransD", "TransR"):
        bad = ok.Config()
        bad.set_work_threads(4); bad.set_dimension(32); bad.set_ent_neg_rate(N); bad.set_nbatches(10)
        bad.set_shared_negatives(P)
        bad.init_from_arrays(E, R, *graph())
        with pytest.raises(ok.KgeError, match="TransE only"):
            bad.set_model_and_session(getattr(ok, model))
