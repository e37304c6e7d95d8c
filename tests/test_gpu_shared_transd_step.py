"""TransD training on shared negatives over RELATION-GROUPED chunks through Config.train_step (Config.set_shared_negatives(...,
by_relation=True) with the TransD model; NON-PARITY, opt-in), untyped and with type-constrained sampling.

In the manner of tests/test_gpu_shared_transh_step.py: every step is compared with torch_ref.loss_and_grads("transd", ...) in
fp64 on the EXPANDED batch -- negative k of sorted position b spelled out as (h_b, c_k, r_b) or (c_k, t_b, r_b), a masked pair
spelled as the positive itself (hinge = margin, gradient exactly zero; the constant is taken off the loss) -- through the test
modules' fp32 restatements of the optimizer rules on the rows the definition lists (tests/shared_transd_ref.py: an entity's
ent_embeddings AND ent_transfer row when its count vector is nonzero, a relation's rel_embeddings row when the chunk's r count is
nonzero, its rel_transfer row when the chunk has any entity record).  The loss is within 1e-5 relative and every one of the four
tables within 1e-5 of that step's largest move of that table.

NOTHING IS EXCUSED.  Before a step's result is compared, the fp64 reference must find no unmasked hinge within 1e-5 of its kink
and no element of a scored triple within 1e-6 of zero (shared_transd_ref.forward min_kink / min_sign, asserted); TABLE_SEEDS holds
initialisation seeds under which that is so in all three steps of each run.

The rates (RATES) are chosen so that 1e-5 of every table's largest move is at least one fp32 ulp of that table's largest stored
element -- below that the comparison would test fp32 storage, not the step (tests/test_gpu_shared_transh_step.py ALPHA_SGD).  The
two transfer tables have the smallest gradients (d x, and the sum of a gxp), and rel_transfer the largest elements (up to 0.52,
an ulp of 6e-8).  Measured on an MI355X at TransH's rates (SGD 0.5, Adagrad 0.05), 1e-5 of rel_transfer's largest move was
4.9e-8 to 9.6e-8 under SGD and 1.5e-8 to 3.0e-8 under Adagrad: at or under that ulp (the steps still passed, with differences of
up to 3.0e-8 and 1.5e-8).  So SGD runs at 1.0 and Adagrad at 0.5, LazyAdam keeps 0.05, and then the smallest bound of any table in
any step of the seven runs was 1.64 ulps (ent_transfer never fell under, at either set of rates).  No table is bounded by its
ulp: all four are held to 1e-5 of the move alone, and every figure is printed before it is judged.

A row without a record keeps every bit, in all four tables and in the slot tables.  LazyAdam runs at adam_epsilon = 1e-4
(tests/test_gpu_shared_step.py ADAM_EPS has the reasoning).  Then: width 50, two runs are bit-identical, a resumed run repeats the
interrupted one bit for bit, by_relation=False and two ranks are refused, and a TransD Config with the option off is untouched."""
import os
import sys

import numpy as np
import pytest

import shared_transd_ref as dref
from conftest import ROOT
from test_gpu_shared_step import ADAM_EPS, ALPHA, E, MARGIN, N, P, R, SEED, graph, same_bits, state
from test_gpu_shared_transh_step import step_lists

pytestmark = pytest.mark.gpu

D = 32
# The rates of the runs compared with the reference, chosen so that 1e-5 of every table's largest move is at least one fp32 ulp of
# that table's largest stored element (module docstring): LazyAdam moves every touched element by about its rate and keeps 0.05.
RATES = {"SGD": 1.0, "LazyAdam": ALPHA, "Adagrad": 0.5}
TABLES = dref.TABLES      # the engine's order: slot table i belongs to TABLES[i]
# initialisation seeds under which the fp64 reference meets the kink and the sign condition in all three steps (found by running
# measure_step three times over seeds 1, 2, ... and keeping the first that does; the conditions are asserted again in every run)
TABLE_SEEDS = {("SGD", False): 1, ("SGD", True): 1, ("LazyAdam", False): 1, ("LazyAdam", True): 1, ("Adagrad", False): 1, ("Adagrad", True): 1}
TABLE_SEED_50 = 1


def make_config(opt, D=D, typed=False, by_relation=True, table_seed=3, chunk=P, seed=SEED, shared=True, mention=True):
    import openkeonspark_amd as ok
    con = ok.Config()
    con.set_work_threads(4); con.set_bern(1); con.set_dimension(D); con.set_ent_neg_rate(N); con.set_rel_neg_rate(0)
    con.set_alpha(RATES.get(opt, ALPHA)); con.set_margin(MARGIN); con.set_opt_method(opt); con.set_nbatches(10)
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
    con.set_model_and_session(ok.TransD)
    return con


def reference_step(con, s0, step, lr_t):
    """The tables (and slots) the definition gives from state s0 for the step `con` has just trained."""
    from torch_ref import loss_and_grads
    from test_gpu_adagrad import adagrad_rule_fp32
    import test_gpu_lazy_rows
    from test_gpu_lazy_rows import adam_rule_fp32
    D, B = con.hidden_size, con.batch_size
    h, t, r, cand, pair, chunks = step_lists(con, step)
    params = {name: s0[name] for name in TABLES}
    denom = B * N
    want = dref.forward(params["ent_embeddings"], params["rel_embeddings"], params["rel_transfer"], params["ent_transfer"], h, t, r, cand,
                        pair, chunks, MARGIN, denom, B)
    bh, bt, br = dref.expand(h, t, r, cand, pair, chunks, B)
    loss, g = loss_and_grads("transd", params, bh, bt, br, B, N, MARGIN, D, D)
    loss -= ((pair & 2) != 0).sum() * MARGIN / denom
    assert abs(loss - want["loss"]) <= 1e-9 * max(abs(loss), 1e-9)      # (the two restatements of the definition agree)
    listed = dref.touched_rows(want["keys"], E, R, B)
    mine = dref.table_gradients(want["keys"], want["records"], E, R, B)
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
            p1[rows], a1[rows], _ = adagrad_rule_fp32(p0[rows], a1[rows], gi[rows], RATES["Adagrad"])
            out["a%d" % i] = a1
        else:
            p1[rows] = (p0[rows] - np.float32(RATES["SGD"]) * gi[rows]).astype(np.float32)
        out[name] = p1
    return loss, out, listed, want, (r, cand, pair, chunks)


def measure_step(con, step, label, typed=False, lists=None):
    """Trains one step and returns its figures against the definition, printed, none of them judged here: min_kink, min_sign,
    loss_err (relative), tables {name: (largest move, largest difference, bound)}, untouched (do rows without a record, in tables
    and slot tables, keep every bit?), from_list (typed candidates checked against their lists)."""
    s0 = state(con)
    lr_t = float(con._adam_lr_t()) if con._lazy_adam else 0.0
    got_loss = con.train_step()
    assert con.global_step == step + 1
    s1 = state(con)
    loss, want, listed, fwd, (r, cand, pair, chunks) = reference_step(con, s0, step, lr_t)
    print("%s step %d: loss %.7f (fp64 %.7f), %d chunks for %d positives, masked pairs %d, listed rows %s, min kink %.2e, min sign %.2e"
          % (label, step, got_loss, loss, len(chunks), len(r), int(((pair & 2) != 0).sum()), [len(listed[n]) for n in TABLES],
             fwd["min_kink"], fwd["min_sign"]))
    from_list = 0
    if typed:      # a candidate of a relation with a list on its side lies in it
        head_off, head_ids, tail_off, tail_ids = lists
        for j, (b0, n) in enumerate(chunks):
            rho = int(r[b0])
            for k in range(N):
                off, ids = (head_off, head_ids) if pair[b0, k] & 1 else (tail_off, tail_ids)
                lst = ids[off[rho]:off[rho + 1]]
                assert len(lst) and int(cand[j, k]) in lst
                from_list += 1
    out = dict(min_kink=fwd["min_kink"], min_sign=fwd["min_sign"], loss_err=abs(got_loss - loss) / abs(loss), tables={}, untouched=True,
               from_list=from_list, rows=sum(len(listed[n]) for n in TABLES))
    for name in TABLES:
        rows = listed[name]
        rest = np.setdiff1d(np.arange(len(s0[name])), rows)
        out["untouched"] &= np.array_equal(s1[name][rest].view(np.uint32), s0[name][rest].view(np.uint32))
        move = np.abs(want[name].astype(np.float64) - s0[name]).max()
        off = np.abs(s1[name][rows].astype(np.float64) - want[name][rows]).max() if len(rows) else 0.0
        bound = 1e-5 * move
        print("   %s: largest move %.3e, largest difference %.3e (bound %.3e; ulp of the largest stored element %.3e)"
              % (name, move, off, bound, float(np.spacing(np.float32(np.abs(s0[name]).max())))))
        out["tables"][name] = (move, off, bound)
        out["ulps"] = min(out.get("ulps", np.inf), bound / float(np.spacing(np.float32(np.abs(s0[name]).max()))))
    for k in want:
        if k[0] in "mva" and k[1:].isdigit():      # slots: outside the listed rows nothing moves
            rest = np.setdiff1d(np.arange(len(s0[k])), listed[TABLES[int(k[1:])]])
            out["untouched"] &= np.array_equal(s1[k][rest].view(np.uint32), s0[k][rest].view(np.uint32))
    return out


def assert_step(m):
    assert m["min_kink"] >= 1e-5 and m["min_sign"] >= 1e-6, (m["min_kink"], m["min_sign"])      # the reference's conditions come first
    assert m["loss_err"] <= 1e-5
    assert m["untouched"]
    for name, (move, off, bound) in m["tables"].items():
        assert off <= bound, (name, off, bound, move)


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_three_steps_follow_the_definition(opt, typed):
    con = make_config(opt, typed=typed, table_seed=TABLE_SEEDS[opt, typed])
    assert con.sparse_inplace and not con.sparse_rows and not con.use_counts and not con.persistent_supported() and con._grads == []
    assert bool(con.lib.kge_typed_sampling()) == typed
    lists = con.type_constraints() if typed else None
    from_list = rows = 0
    for step in range(3):
        m = measure_step(con, step, "%s typed %d" % (opt, typed), typed, lists)
        assert_step(m)
        from_list += m["from_list"]; rows += m["rows"]
    assert (from_list > 0) == typed and rows > 0


def test_a_width_off_the_vector_path():
    """Width 50: the emit kernel's scalar loads and stores; one SGD step against the definition."""
    con = make_config("SGD", D=50, typed=True, table_seed=TABLE_SEED_50)
    assert_step(measure_step(con, 0, "width 50", True, con.type_constraints()))


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
    assert [int(x) for x in np.load(ckpt)["shared_negatives"]] == [P, SEED, 1, 1]      # the checkpoint record is the TransE / TransH one
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
    assert "by_relation=True" in str(exc.value) and "TransD" in str(exc.value)
    with pytest.raises(ok.KgeError, match="SGD, LazyAdam or Adagrad"):
        make_config("Adam")


@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_with_the_option_off_a_transd_step_is_untouched(opt):
    """set_shared_negatives(0) against a Config that never names the feature: the unshared touched-rows TransD step, with none of
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
    mp.start_processes(_two_rank_worker, args=(2, 36100 + os.getpid() % 1000, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    for rank in range(2):
        said = open(os.path.join(str(tmp_path), "said_%d.txt" % rank)).read()
        assert "one rank only" in said and "global order" in said and "2 ranks" in said, said
