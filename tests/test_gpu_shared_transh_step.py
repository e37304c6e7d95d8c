"""TransH training on shared negatives over RELATION-GROUPED chunks through Config.train_step (Config.set_shared_negatives(...,
by_relation=True) with the TransH model; NON-PARITY, opt-in), untyped and with type-constrained sampling.

In the manner of tests/test_gpu_shared_grouped_step.py: every step is compared with torch_ref.loss_and_grads("transh", ...) in
fp64 on the EXPANDED batch -- negative k of sorted position b spelled out as (h_b, c_k, r_b) or (c_k, t_b, r_b), a masked pair
spelled as the positive itself (hinge = margin, gradient exactly zero; the constant is taken off the loss) -- through the test
modules' fp32 restatements of the optimizer rules on the rows the definition lists (tests/shared_transh_ref.py: an entity row
with a nonzero count vector, a relation's rel_embeddings row when the chunk's r count is nonzero, its normal_vectors row when the
chunk has any entity record).  A table may differ from the result by 1e-5 of the step's largest move, except in rows
torch_ref.near_kink_rows excuses; the fp64 reference alone may excuse at most 1 % of the touched rows.  A row without a record
keeps every bit, in all three tables and in the slot tables.  LazyAdam runs at adam_epsilon = 1e-4 (tests/test_gpu_shared_step.py
ADAM_EPS has the reasoning).  Then: width 50, two runs are bit-identical, a resumed run repeats the interrupted one bit for bit,
a resume under another chunk, seed or by_relation is refused, by_relation=False and two ranks are refused, and a TransH Config
with the option off is untouched by it."""
import os
import sys

import numpy as np
import pytest

import shared_transh_ref as tref
from conftest import ROOT, parity_report
from test_gpu_shared_step import ADAM_EPS, ALPHA, E, MARGIN, N, P, R, SEED, graph, same_bits, state

pytestmark = pytest.mark.gpu

D = 32
TABLES = ("ent_embeddings", "rel_embeddings", "normal_vectors")
# initialisation seeds of the runs compared with the fp64 reference: chosen, as tests/test_gpu_shared_grouped_step.py TABLE_SEED is,
# so that the REFERENCE finds no element of h^ + r^ - t^ within 1e-6 of zero in the three steps of any of the six runs (one such
# element excuses the rows of its group, more than 1 % of the rows three steps touch)
TABLE_SEED, TABLE_SEED_50 = 7, 5
# SGD's learning rate in the runs compared with the reference.  normal_vectors is a [6, 32] table drawn with sigma = sqrt(2.6 / 38)
# = 0.26 and cut at two sigma, so its elements reach 0.52 and are stored with an ulp of up to 6e-8: two correct fp32 evaluations of
# p - lr g may differ by that much.  Its gradient is a sum of small cross terms (d x + a gxp), about 0.03 at this batch, so at the
# 0.05 of tests/test_gpu_shared_step.py the step's largest move is 1.7e-3 and the bound of 1e-5 of it, 1.7e-8, lies BELOW one ulp
# of the stored value: the comparison would test fp32 storage, not the step (seen: differences of exactly one ulp, 2.98e-8).
# At 0.5 the bound is 1.7e-7, three ulps.  LazyAdam and Adagrad move every touched element by about the rate itself and keep 0.05.
ALPHA_SGD = 0.5


def alpha_of(opt):
    return ALPHA_SGD if opt == "SGD" else ALPHA


def make_config(opt, D=D, typed=False, by_relation=True, table_seed=3, chunk=P, seed=SEED, shared=True, mention=True):
    import openkeonspark_amd as ok
    con = ok.Config()
    con.set_work_threads(4); con.set_bern(1); con.set_dimension(D); con.set_ent_neg_rate(N); con.set_rel_neg_rate(0)
    con.set_alpha(alpha_of(opt)); con.set_margin(MARGIN); con.set_opt_method(opt); con.set_nbatches(10)
    con.sparse_rows = True
    con.seed = table_seed
    con.adam_epsilon = ADAM_EPS
    if shared:
        con.set_shared_negatives(chunk, seed=seed, by_relation=by_relation)
    elif mention:
        con.set_shared_negatives(0)
    con.lib.kge_set_option(b"libc_rand_restart", 1)
    con.init_from_arrays(E, R, *graph())
    empty = (np.zeros(0, np.int64),) * 3      # (also drops the lists an earlier engine of the process left)
    con.init_evaluation_from_arrays(empty, empty, derive_types=typed)
    con.set_type_constrained_sampling(typed)
    con.set_model_and_session(ok.TransH)
    return con


def step_lists(con, step):
    """The step's sorted positives and the lists, checked against the host statement of the order."""
    from openkeonspark_amd.train_paths import shared_chunk_cap, shared_relation_chunks
    B = con.batch_size
    cand, pair, perm, chunks = con.shared_negatives_of(step)
    pos = con._sparse_buf["shared_batch"].cpu().numpy()[:, :B].astype(np.int64)
    want_perm, want_chunks, n_chunks = shared_relation_chunks(pos[2], P, R)
    assert np.array_equal(perm, want_perm) and np.array_equal(chunks, want_chunks[:n_chunks])
    assert cand.shape == (n_chunks, N) and pair.shape == (B, N) and len(want_chunks) == shared_chunk_cap(B, P, R)
    h, t, r = pos[:, perm]
    assert all(len(set(r[b0:b0 + n].tolist())) == 1 for b0, n in chunks)
    return h, t, r, cand, pair, chunks


def reference_step(con, s0, step, lr_t):
    from torch_ref import loss_and_grads, near_kink_rows
    from test_gpu_adagrad import adagrad_rule_fp32
    import test_gpu_lazy_rows
    from test_gpu_lazy_rows import adam_rule_fp32
    D, B = con.hidden_size, con.batch_size
    h, t, r, cand, pair, chunks = step_lists(con, step)
    params = {name: s0[name] for name in TABLES}
    denom = B * N
    want = tref.forward(params["ent_embeddings"], params["rel_embeddings"], params["normal_vectors"], h, t, r, cand, pair, chunks, MARGIN,
                        denom, B)
    bh, bt, br = tref.expand(h, t, r, cand, pair, chunks, B)
    loss, g = loss_and_grads("transh", params, bh, bt, br, B, N, MARGIN, D, D)
    loss -= ((pair & 2) != 0).sum() * MARGIN / denom
    assert abs(loss - want["loss"]) <= 1e-9 * max(abs(loss), 1e-9)      # (the two restatements of the definition agree)
    listed = tref.touched_rows(want["keys"], E, R, B)
    mine = tref.table_gradients(want["keys"], want["records"], E, R, B)
    out = {}
    for i, name in enumerate(TABLES):
        p0, gi, rows = s0[name], g[name].astype(np.float32), listed[name]
        assert np.abs(g[name] - mine[name]).max() <= 1e-9 * np.abs(g[name]).max()      # (... on every row of every table)
        assert np.abs(g[name][np.setdiff1d(np.arange(len(p0)), rows)]).max(initial=0.0) <= 1e-12      # no gradient outside the listed rows
        p1 = p0.copy()
        if con._lazy_adam:
            m1, v1 = s0["m%d" % i].copy(), s0["v%d" % i].copy()
            eps0, test_gpu_lazy_rows.EPS = test_gpu_lazy_rows.EPS, ADAM_EPS
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
            p1[rows] = (p0[rows] - np.float32(ALPHA_SGD) * gi[rows]).astype(np.float32)
        out[name] = p1
    excused, near = near_kink_rows("transh", params, bh, bt, br, B, N, D, D, tol=1e-6)
    return loss, out, listed, excused, near, want, (r, cand, pair, chunks)


def run_three_steps(con, label, typed=False):
    """Three steps against the definition; returns (touched rows, excused rows, near-zero elements)."""
    lists = con.type_constraints() if typed else None
    touched = excused_n = near_n = from_list = 0
    for step in range(3):
        s0 = state(con)
        lr_t = float(con._adam_lr_t()) if con._lazy_adam else 0.0
        got_loss = con.train_step()
        assert con.global_step == step + 1
        s1 = state(con)
        loss, want, listed, excused, near, fwd, (r, cand, pair, chunks) = reference_step(con, s0, step, lr_t)
        near_n += near
        print("%s step %d: loss %.7f (fp64 %.7f), %d chunks for %d positives, masked pairs %d, listed rows %s, near-zero elements %d, "
              "min kink %.2e" % (label, step, got_loss, loss, len(chunks), len(r), int(((pair & 2) != 0).sum()),
                                 [len(listed[n]) for n in TABLES], near, fwd["min_kink"]))
        if typed:      # a candidate of a relation with a list on its side lies in it
            head_off, head_ids, tail_off, tail_ids = lists
            for j, (b0, n) in enumerate(chunks):
                rho = int(r[b0])
                for k in range(N):
                    off, ids = (head_off, head_ids) if pair[b0, k] & 1 else (tail_off, tail_ids)
                    lst = ids[off[rho]:off[rho + 1]]
                    assert len(lst) and int(cand[j, k]) in lst
                    from_list += 1
        assert fwd["min_kink"] >= 1e-5, fwd["min_kink"]      # no hinge within rounding of its kink
        assert abs(got_loss - loss) <= 1e-5 * abs(loss)
        for name in TABLES:
            rows = listed[name]
            rest = np.setdiff1d(np.arange(len(s0[name])), rows)
            assert np.array_equal(s1[name][rest].view(np.uint32), s0[name][rest].view(np.uint32))      # no record: every bit stays
            ok_rows = np.setdiff1d(rows, np.array(sorted(excused.get(name, ())), dtype=np.int64))
            touched += len(rows); excused_n += len(rows) - len(ok_rows)
            move = np.abs(want[name].astype(np.float64) - s0[name]).max()
            off = np.abs(s1[name][ok_rows].astype(np.float64) - want[name][ok_rows]).max() if len(ok_rows) else 0.0
            print("   %s: largest move %.3e, largest difference %.3e (bound %.3e)" % (name, move, off, 1e-5 * move))
            assert off <= 1e-5 * move, (name, off, move)
        for k in want:
            if k[0] in "mva" and k[1:].isdigit():      # slots: outside the listed rows nothing moves
                rest = np.setdiff1d(np.arange(len(s0[k])), listed[TABLES[int(k[1:])]])
                assert np.array_equal(s1[k][rest].view(np.uint32), s0[k][rest].view(np.uint32))
    assert (from_list > 0) == typed
    return touched, excused_n, near_n


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_three_steps_follow_the_definition(opt, typed):
    con = make_config(opt, typed=typed, table_seed=TABLE_SEED)
    assert con.sparse_inplace and not con.sparse_rows and not con.use_counts and not con.persistent_supported() and con._grads == []
    assert bool(con.lib.kge_typed_sampling()) == typed
    touched, excused_n, _ = run_three_steps(con, "%s typed %d" % (opt, typed), typed)
    parity_report("shared_transh_step_%s_typed%d" % (opt, typed), touched_rows=touched, rows_excused=excused_n)
    assert excused_n <= 0.01 * touched, (excused_n, touched)


def test_a_width_off_the_vector_path():
    """Width 50: the emit kernel's scalar loads and stores; one SGD step against the definition's loss and rows."""
    con = make_config("SGD", D=50, typed=True, table_seed=TABLE_SEED_50)
    s0 = state(con)
    got_loss = con.train_step()
    loss, want, listed, excused, near, fwd, _ = reference_step(con, s0, 0, 0.0)
    s1 = state(con)
    assert fwd["min_kink"] >= 1e-5 and abs(got_loss - loss) <= 1e-5 * abs(loss)
    for name in TABLES:
        ok_rows = np.setdiff1d(listed[name], np.array(sorted(excused.get(name, ())), dtype=np.int64))
        move = np.abs(want[name].astype(np.float64) - s0[name]).max()
        assert np.abs(s1[name][ok_rows].astype(np.float64) - want[name][ok_rows]).max() <= 1e-5 * move
        assert len(ok_rows) >= 0.99 * len(listed[name])


@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_reproducible_and_resumable_bit_for_bit(opt, tmp_path):
    from openkeonspark_amd import distribute_training as dt
    import openkeonspark_amd as ok
    a = make_config(opt, typed=True)
    la = [a.train_step() for _ in range(2)]
    dt.save_checkpoint(a, str(tmp_path))
    la.append(a.train_step())
    b = make_config(opt, typed=True)
    lb = [b.train_step() for _ in range(3)]
    assert la == lb and same_bits(state(a), state(b))
    ckpt = os.path.join(str(tmp_path), "model.ckpt-2.npz")
    assert [int(x) for x in np.load(ckpt)["shared_negatives"]] == [P, SEED, 1, 1]
    c = make_config(opt, typed=True, table_seed=4)
    assert dt.restore_checkpoint(c, ckpt) == 2
    assert c.train_step() == la[2] and same_bits(state(a), state(c))
    # another chunk, another seed, untyped, or the option off: another run, refused
    for kw in (dict(typed=True, chunk=P - 1), dict(typed=True, seed=SEED + 1), dict(typed=False), dict(shared=False)):
        d = make_config(opt, **kw)
        with pytest.raises(ok.KgeError, match="shared negatives"):
            dt.restore_checkpoint(d, ckpt)


def test_chunks_by_position_are_refused_naming_by_relation():
    import openkeonspark_amd as ok
    with pytest.raises(ok.KgeError, match="TransE only") as exc:
        make_config("SGD", by_relation=False)
    assert "by_relation=True" in str(exc.value)
    with pytest.raises(ok.KgeError, match="SGD, LazyAdam or Adagrad"):
        make_config("Adam")


@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_with_the_option_off_a_transh_step_is_untouched(opt):
    """set_shared_negatives(0) against a Config that never names the feature: the unshared touched-rows TransH step, with none of
    the shared step's buffers -- bit for bit under LazyAdam and Adagrad.  The unshared SGD step adds its per-row sums with fp32
    atomics (kge_forward_backward_sgd_rows) and does not repeat its own bits from run to run, so there the first loss, which both
    runs compute from the same tables, is equal and the tables agree to 1e-6.  The shared run from the same state trains on other
    negatives."""
    a = make_config(opt, shared=False)
    la = [a.train_step() for _ in range(3)]
    b = make_config(opt, shared=False, mention=False)
    lb = [b.train_step() for _ in range(3)]
    if opt == "SGD":
        sa, sb = state(a), state(b)
        assert la[0] == lb[0] and all(np.abs(sa[k] - sb[k]).max() <= 1e-6 for k in sa)
    else:
        assert la == lb and same_bits(state(a), state(b))
    assert a.sparse_inplace and a._sparse_buf is None
    c = make_config(opt)
    lc = [c.train_step() for _ in range(3)]
    assert lc != la and "chunks" in c._sparse_buf and len(c.shared_negatives_of(2)) == 4


def _two_rank_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import openkeonspark_amd as ok
    said = "NOT REFUSED"
    try:
        con = make_config("SGD")
        con.init_distributed()
        con.train_step()
    except ok.KgeError as exc:
        said = str(exc)
    with open(os.path.join(out_dir, "said_%d.txt" % rank), "w") as f:
        f.write(said)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_are_refused_with_the_reason(tmp_path):
    import torch.multiprocessing as mp
    mp.start_processes(_two_rank_worker, args=(2, 35100 + os.getpid() % 1000, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    for rank in range(2):
        said = open(os.path.join(str(tmp_path), "said_%d.txt" % rank)).read()
        assert "one rank only" in said and "global order" in said and "2 ranks" in said, said
