"""Training on relation-grouped shared negatives with IN-CHUNK candidates through Config.train_step
(Config.set_shared_negatives(..., by_relation=True, in_chunk=K); include/kge_mi355.h, "In-chunk candidates"), all four models.

The graph and the constants are tests/test_gpu_shared_step.py's (E = 300, R = 6, B = 96, P = 16, N = 4), K = 8: a batch holds about
sixteen positives per relation, so its chunks are full ones of 16 and short remainders, both shorter and longer than K (asserted in
every run).  In the manner of tests/test_gpu_shared_grouped_step.py every step is compared with the fp64 restatements that exist,
driven by the N + K wide lists Config.shared_negatives_of returns (tests/shared_in_chunk_ref.py reference_step): the loss within
1e-5, every table within 1e-5 of the step's largest move except in rows torch_ref.near_kink_rows excuses, of which the fp64
reference alone may excuse at most 1 % of the touched rows; a row without a record keeps every bit.  The device's lists themselves
must be the host statement's (shared_in_chunk_ref.host_lists) of the step's positives.

Rates: TransE 0.05 as its existing tests; TransH and TransD SGD 0.5 (tests/test_gpu_shared_transh_step.py ALPHA_SGD has the
reasoning: 1e-5 of the largest move must not fall under an ulp of the stored values); TransR SGD 1.0 (tests/
test_gpu_shared_transr_step.py RATES).  LazyAdam at adam_epsilon = 1e-4 (tests/test_gpu_shared_step.py ADAM_EPS).

TABLE_SEEDS: in-chunk candidates are the graph's own heads and tails, so the initialisation seeds were searched afresh, on the
CPU, by tools/shared_in_chunk_seeds.py: it replays the sampler with the CPU oracle, states the lists with host_lists and walks the
steps with reference_step, and keeps the first seed of 1, 2, ... under which the fp64 reference finds no element of a scored
triple within 1e-6 of zero and no hinge within 1e-5 of its kink in any step of the run.  The search result (seed: near-zero
elements over the run's steps): TransE SGD typed 1: 1, 2: 1, 3: 1, 4: 0; every other run 1: 0 (TransE SGD untyped, LazyAdam and
Adagrad untyped and typed, three steps each; TransE SGD typed at width 50, one step; TransH and TransD SGD, three steps; TransR
SGD, one step).  So no row is expected to be excused at all (one near-zero element would excuse the rows of its group, about
fifteen of the ~600 a run touches); the old files' seeds (13, 7, 5) were not reused.  The TransE runs check that the positives the device drew are the oracle's, and every run that
the device's lists are host_lists', so the search saw the lists the device trains on."""
import os

import numpy as np
import pytest

import shared_in_chunk_ref as icref
from conftest import parity_report
from test_gpu_shared_step import ADAM_EPS, ALPHA, E, MARGIN, N, P, R, SEED, graph, same_bits, state

pytestmark = pytest.mark.gpu

D, K = 32, 8
NT = N + K
RATES = {("transe", "SGD"): ALPHA, ("transe", "LazyAdam"): ALPHA, ("transe", "Adagrad"): ALPHA, ("transh", "SGD"): 0.5,
         ("transd", "SGD"): 0.5, ("transr", "SGD"): 1.0}
TABLE_SEEDS = {("transe", "SGD", False): 1, ("transe", "SGD", True): 4, ("transe", "LazyAdam", False): 1, ("transe", "LazyAdam", True): 1,
               ("transe", "Adagrad", False): 1, ("transe", "Adagrad", True): 1, ("transh", "SGD", False): 1, ("transd", "SGD", False): 1,
               ("transr", "SGD", False): 1}
TABLE_SEED_50 = 1


def make_config(model, opt, D=D, typed=False, in_chunk=K, table_seed=3, say_in_chunk=True):
    import openkeonspark_amd as ok
    con = ok.Config()
    con.set_work_threads(4); con.set_bern(1); con.set_dimension(D); con.set_ent_neg_rate(N); con.set_rel_neg_rate(0)
    con.set_alpha(RATES[model, opt]); con.set_margin(MARGIN); con.set_opt_method(opt); con.set_nbatches(10)
    if model != "transr":
        con.sparse_rows = True
    con.seed = table_seed
    con.adam_epsilon = ADAM_EPS
    if say_in_chunk:
        con.set_shared_negatives(P, seed=SEED, by_relation=True, in_chunk=in_chunk)
    else:
        con.set_shared_negatives(P, seed=SEED, by_relation=True)
    con.lib.kge_set_option(b"libc_rand_restart", 1)
    con.init_from_arrays(E, R, *graph())
    empty = (np.zeros(0, np.int64),) * 3      # (also drops the lists an earlier engine of the process left)
    con.init_evaluation_from_arrays(empty, empty, derive_types=typed)
    con.set_type_constrained_sampling(typed)
    con.set_model_and_session({"transe": ok.TransE, "transh": ok.TransH, "transd": ok.TransD, "transr": ok.TransR}[model])
    return con


def bern_table(con):
    out = np.zeros(R, np.float32)
    assert con.lib.kge_index_copy(b"bern_prob", out.ctypes.data, out.nbytes) == out.nbytes
    return out


TRAIN = set(zip(*[a.tolist() for a in graph()]))


def step_lists(con, step, typed):
    """The step's sorted positives and its lists N + K wide, which must be the host statement's of the step's positives."""
    B = con.batch_size
    cand, pair, perm, chunks = con.shared_negatives_of(step)
    pos = con._sparse_buf["shared_batch"].cpu().numpy()[:, :B].astype(np.int64)
    h2, t2, r2, want_cand, want_pair, want_perm, want_chunks = icref.host_lists(
        pos[0], pos[1], pos[2], P, E, R, N, K, SEED, step, TRAIN, bern_table(con), con.type_constraints() if typed else None)
    if typed:      # (the lists the seed search derives on the host are the engine's)
        assert all(np.array_equal(x, y) for x, y in zip(con.type_constraints(), icref.derived_type_lists(*graph(), R)))
    assert cand.shape == (len(chunks), NT) and pair.shape == (B, NT)
    assert np.array_equal(perm, want_perm) and np.array_equal(chunks, want_chunks)
    assert np.array_equal(cand, want_cand) and np.array_equal(pair, want_pair)
    assert np.array_equal(con._sparse_buf["sorted"].cpu().numpy()[:, :B], pos[:, perm])
    # the batch holds chunks both shorter and longer than K: columns that end in -1 and columns that rotate
    assert chunks[:, 1].min() < K < chunks[:, 1].max()
    short = chunks[:, 1] < K
    assert (cand[short][:, NT - 1] == -1).all() and (cand[~short][:, N:] >= 0).all()
    return pos, (h2, t2, r2, cand, pair, chunks)


def run_steps(con, model, opt, n_steps, typed, label, oracle_kg=None):
    """n_steps against the definition; returns (touched rows, excused rows, near-zero elements)."""
    tables = icref.TABLES[model]
    touched = excused_n = near_n = 0
    for step in range(n_steps):
        s0 = state(con)
        lr_t = float(con._adam_lr_t()) if con._lazy_adam else 0.0
        got_loss = con.train_step()
        assert con.global_step == step + 1
        s1 = state(con)
        pos, lists = step_lists(con, step, typed)
        if oracle_kg is not None:      # (the seed search replays the sampler with the CPU oracle: it saw these positives)
            oh, ot, orl, _ = oracle_kg.sampling(con.batch_size, 0, 0)
            assert np.array_equal(pos, np.stack([oh, ot, orl]))
        w = icref.reference_step(model, opt, s0, lists, lr_t, RATES[model, opt], E, R, MARGIN, ADAM_EPS)
        cand, pair = lists[3], lists[4]
        near_n += w["near"]
        print("%s step %d: loss %.7f (fp64 %.7f), %d chunks, masked pairs drawn %d in-chunk %d, -1 columns %d, listed rows %s, near-zero "
              "elements %d, min kink %.2e" % (label, step, got_loss, w["loss"], len(lists[5]), int(((pair[:, :N] & 2) != 0).sum()),
                                              int(((pair[:, N:] & 2) != 0).sum()), int((cand < 0).sum()),
                                              [len(w["listed"][n]) for n in tables], w["near"], w["min_kink"]))
        assert w["min_kink"] >= 1e-5, w["min_kink"]      # no hinge within rounding of its kink
        assert abs(got_loss - w["loss"]) <= 1e-5 * abs(w["loss"])
        for i, name in enumerate(tables):
            rows = w["listed"][name]
            rest = np.setdiff1d(np.arange(len(s0[name])), rows)
            for k in [name] + [s + str(i) for s in "mva" if s + str(i) in s0]:      # no record: every bit stays, slots too
                assert np.array_equal(s1[k][rest].view(np.uint32), s0[k][rest].view(np.uint32)), k
            ok_rows = np.setdiff1d(rows, np.array(sorted(w["excused"].get(name, ())), dtype=np.int64))
            touched += len(rows); excused_n += len(rows) - len(ok_rows)
            move = np.abs(w["state"][name].astype(np.float64) - s0[name]).max()
            off = np.abs(s1[name][ok_rows].astype(np.float64) - w["state"][name][ok_rows]).max() if len(ok_rows) else 0.0
            print("   %s: largest move %.3e, largest difference %.3e (bound %.3e)" % (name, move, off, 1e-5 * move))
            assert off <= 1e-5 * move, (name, off, move)
    return touched, excused_n, near_n


def oracle_sampler():
    from oracle import oracle
    h, t, r = graph()
    return oracle.KG(arrays=(E, R, h, t, r, 0), work_threads=4, bern=1)


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
def test_transe_three_steps_follow_the_definition(opt, typed):
    con = make_config("transe", opt, typed=typed, table_seed=TABLE_SEEDS["transe", opt, typed])
    assert con.sparse_rows and con.use_counts and not con.persistent_supported() and con._grads == []
    assert bool(con.lib.kge_typed_sampling()) == typed
    kg = oracle_sampler()
    kg.set_stream_states(con.get_stream_states())
    touched, excused_n, _ = run_steps(con, "transe", opt, 3, typed, "transe %s typed %d" % (opt, typed), kg)
    parity_report("shared_in_chunk_step_%s_typed%d" % (opt, typed), touched_rows=touched, rows_excused=excused_n)
    assert excused_n <= 0.01 * touched, (excused_n, touched)


@pytest.mark.parametrize("model", ["transh", "transd"])
def test_transh_and_transd_three_sgd_steps_follow_the_definition(model):
    con = make_config(model, "SGD", table_seed=TABLE_SEEDS[model, "SGD", False])
    assert con.sparse_inplace and not con.sparse_rows and con._grads == []
    touched, excused_n, _ = run_steps(con, model, "SGD", 3, False, model + " SGD")
    assert excused_n <= 0.01 * touched, (excused_n, touched)


def test_transr_one_sgd_step_follows_the_definition():
    """The -1 columns of a short chunk go through the row GEMMs as row 0 and get no gradient (csrc/shared_transr.hip
    shared_transr_jobs_kernel): the dense gradient tables must still be the definition's."""
    con = make_config("transr", "SGD", table_seed=TABLE_SEEDS["transr", "SGD", False])
    assert not con.sparse_inplace and not con.sparse_rows and len(con._grads) == 3
    touched, excused_n, _ = run_steps(con, "transr", "SGD", 1, False, "transr SGD")
    assert excused_n <= 0.01 * touched, (excused_n, touched)
    assert all(not g.any() for g in con.get_gradients().values())      # the gradient tables are zero between steps


def test_a_width_off_the_vector_path():
    """Width 50: the emit kernel's scalar loads and the unfused reduce; one typed TransE SGD step."""
    con = make_config("transe", "SGD", D=50, typed=True, table_seed=TABLE_SEED_50)
    touched, excused_n, _ = run_steps(con, "transe", "SGD", 1, True, "transe SGD width 50")
    assert excused_n <= 0.01 * touched, (excused_n, touched)


@pytest.mark.parametrize("model", ["transe", "transh", "transd"])
def test_reproducible_and_resumable_bit_for_bit(model, tmp_path):
    from openkeonspark_amd import distribute_training as dt
    import openkeonspark_amd as ok
    a = make_config(model, "SGD", typed=True)
    la = [a.train_step() for _ in range(2)]
    dt.save_checkpoint(a, str(tmp_path))
    la.append(a.train_step())
    b = make_config(model, "SGD", typed=True)
    lb = [b.train_step() for _ in range(3)]
    assert la == lb and same_bits(state(a), state(b))
    ckpt = os.path.join(str(tmp_path), "model.ckpt-2.npz")
    assert [int(x) for x in np.load(ckpt)["shared_negatives"]] == [P, SEED, 1, 1, K]
    c = make_config(model, "SGD", typed=True, table_seed=4)
    assert dt.restore_checkpoint(c, ckpt) == 2
    assert c.train_step() == la[2] and same_bits(state(a), state(c))
    # another K, or none: another run, refused, and the flag is named
    for kw in (dict(in_chunk=K + 1), dict(in_chunk=0)):
        d = make_config(model, "SGD", typed=True, **kw)
        with pytest.raises(ok.KgeError, match="--shared_negatives_in_chunk"):
            dt.restore_checkpoint(d, ckpt)


@pytest.mark.parametrize("model,opt", [("transe", "SGD"), ("transe", "LazyAdam"), ("transe", "Adagrad"), ("transh", "SGD"), ("transd", "SGD")])
def test_in_chunk_zero_is_the_grouped_step_bit_for_bit(model, opt, tmp_path):
    """in_chunk=0 against a Config that never names the keyword: tables, slots and losses bit for bit, lists N wide, the checkpoint
    record four fields long.  The run with K candidates from the same state trains on other negatives."""
    from openkeonspark_amd import distribute_training as dt
    a = make_config(model, opt, typed=True, in_chunk=0)
    la = [a.train_step() for _ in range(3)]
    b = make_config(model, opt, typed=True, say_in_chunk=False)
    lb = [b.train_step() for _ in range(3)]
    assert la == lb and same_bits(state(a), state(b))
    for x, y in zip(a.shared_negatives_of(2), b.shared_negatives_of(2)):
        assert np.array_equal(x, y)
    assert a.shared_negatives_of(2)[0].shape[1] == N and a._sparse_buf["pair"].shape[1] == N
    assert dt.shared_negatives_record(a).tolist() == [P, SEED, 1, 1]
    c = make_config(model, opt, typed=True)
    lc = [c.train_step() for _ in range(3)]
    assert lc != la and c.shared_negatives_of(2)[0].shape[1] == NT
    # ... whose drawn columns are the same candidates and sides
    assert np.array_equal(c.shared_negatives_of(2)[0][:, :N], a.shared_negatives_of(2)[0])
    assert np.array_equal(c.shared_negatives_of(2)[1][:, :N] & 1, a.shared_negatives_of(2)[1] & 1)
