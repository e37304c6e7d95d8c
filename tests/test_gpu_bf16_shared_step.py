"""Shared negatives on bf16 tables through Config.train_step (set_table_dtype("bf16") with set_shared_negatives, either order):
a synthetic graph of 300 entities, B = 96, P = 16, N = 5, widths 8 and 200, SGD and RowAdagrad; chunks by position, by relation,
and by relation with typed candidates and in_chunk = 2.

Every step is replayed on the host from the device's tables before it.  BEFORE the step runs, the replay draws the step's
positives again (the sampler's streams are put back), builds the lists from the host statements of the draw
(tests/shared_neg_ref.py, tests/shared_in_chunk_ref.py host_lists), runs the fp64 definition on the widened tables
(shared_neg_ref.forward / test_gpu_shared_emit_chunks.forward_chunks) and asserts test_gpu_shared_emit's conditions -- no hinge
within 1e-4 of its kink, no element |e| < 1e-5 in a scored triple -- so the row lists and int32 counts of shared_neg_ref.reduce
(keys in the [0, E) + [E, E + R) row space) are exact and NO ROW IS EXCUSED.  The tables are the lattice of
tests/test_gpu_shared_emit.py through set_parameters (random rows cannot meet the sign condition); the rates are small enough
that three steps move no element by more than a few bf16 ulps, which the lattice's gaps absorb.  The lattice seeds were chosen
by replaying these runs on the CPU alone (tools/bf16_shared_seeds.py: the oracle's sampler, the same host lists, the fp64 rule).

After the step: the device's lists are the host's; the loss is the definition's to 1e-5; rows without a record, rows whose counts
cancel and every RowAdagrad accumulator outside the listed rows keep their bits.  The stored rows are checked twice:
  * against bf16_ref.update (fp64) stored by bf16_ref.round_rows' hash, by the rule of tests/test_gpu_bf16_apply.py -- the device
    forms y in fp32, a few ulps from the fp64 y, so every stored value must be one of y's two bf16 neighbours and must be the
    hash's pick wherever frac * 65536 + rnd is not within 4 of a multiple of 65536; the share of elements that band leaves
    undecided is computed from the reference alone before the comparison and must be at most 1e-3;
  * bit for bit, every element of every row, against kge_transe_apply_rows_*_bf16 called by hand on the pre-step tables with the
    HOST's row list and counts (that kernel alone is held to the rule above by tests/test_gpu_bf16_apply.py).
An fp64 replay cannot be compared bit for bit by itself: one element in about 4000 is stored differently by an fp32 and an fp64 y.

Then: two runs are bit-identical; two steps, checkpoint, resume, two steps equal four steps, and another rounding seed or chunk is
refused; an fp32 shared run and an unshared bf16 run give the same bits before and after a bf16 + shared run in the process."""
import ctypes

import numpy as np
import pytest

import bf16_ref
import shared_neg_ref as ref

pytestmark = pytest.mark.gpu

E, R, B = 300, 6, 96
P, N, MARGIN = 16, 5, 1.0
SHARED_SEED, ROUND_SEED = 12345, 0xB16B00B5
RATES = {"SGD": 0.01, "RowAdagrad": 0.003}
BAND = 4
MODES = {"position": dict(), "relation": dict(by_relation=True), "typed_in_chunk": dict(by_relation=True, in_chunk=2)}
# lattice seeds of the runs: the first of 1, 2, ... whose CPU replay (tools/bf16_shared_seeds.py) keeps every hinge 5e-4 from its kink
# and every element 1e-3 from zero in all three steps; 1 where a run is not listed
TABLE_SEEDS = {(8, "SGD", "relation"): 5, (200, "SGD", "relation"): 2, (200, "RowAdagrad", "relation"): 2}


def graph():
    from openkeonspark_amd.synthetic import generate_triples
    h, t, r = generate_triples(E, R, 10 * B, seed=7)
    return h.astype(np.int64), t.astype(np.int64), r.astype(np.int64)


def lattice(D, seed):
    """tests/test_gpu_shared_emit.py lattice_tables for this graph's E and R."""
    rng = np.random.default_rng(seed)
    mags = np.array([1.0] * (D - D // 2) + [3.0] * (D // 2))
    ent = np.stack([rng.permutation(mags) for _ in range(E)]) * rng.choice([-1.0, 1.0], (E, D)) * 0.1
    rel = rng.choice([-1.0, 1.0], (R, D)) * 0.07
    return ent.astype(np.float32), rel.astype(np.float32)


def configure(con, D, opt, mode, bf16=True, shared=True, bf16_first=True, round_seed=ROUND_SEED, chunk=P):
    """The setters of a run, up to init_from_arrays (shared by the CPU seed search)."""
    kw = MODES[mode]
    con.set_work_threads(4); con.set_bern(0); con.set_dimension(D); con.set_ent_neg_rate(N); con.set_rel_neg_rate(0)
    con.set_alpha(RATES[opt]); con.set_margin(MARGIN); con.set_opt_method(opt); con.set_nbatches(10)
    con.sparse_rows = True
    calls = [lambda: con.set_table_dtype("bf16", seed=round_seed) if bf16 else None,
             lambda: con.set_shared_negatives(chunk, seed=SHARED_SEED, **kw) if shared else None]
    for call in calls if bf16_first else calls[::-1]:
        call()
    con.lib.kge_set_option(b"libc_rand_restart", 1)
    con.init_from_arrays(E, R, *graph())
    assert con.batch_size == B


def make_config(D, opt, mode, table_seed=None, **kw):
    import openkeonspark_amd as ok
    con = ok.Config()
    configure(con, D, opt, mode, **kw)
    typed = mode == "typed_in_chunk" and kw.get("shared", True)
    empty = (np.zeros(0, np.int64),) * 3      # (also drops the lists an earlier engine of the process left)
    con.init_evaluation_from_arrays(empty, empty, derive_types=typed)
    con.set_type_constrained_sampling(typed)
    con.set_model_and_session(ok.TransE)
    ent, rel = lattice(D, TABLE_SEEDS.get((D, opt, mode), 1) if table_seed is None else table_seed)
    con.set_parameters({"ent_embeddings": ent, "rel_embeddings": rel})
    return con


def bits(t):
    import torch
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16).copy()


def state(con):
    """Every trained bit of a run: bf16 tables as uint16, fp32 tables as uint32, accumulators as uint32."""
    out = [bits(t) if t.element_size() == 2 else t.detach().cpu().numpy().view(np.uint32).copy() for t in con._tables]
    if con._row_adagrad:
        out += [a.detach().cpu().numpy().view(np.uint32).copy() for a in con._rowadagrad_acc]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


TRAIN = None


def host_step(full, acc, pos, step, mode, opt, type_lists=None):
    """One step of the definition from the stored tables `full` (uint16 [E + R, D]) and the accumulators `acc` (fp32 [E + R] or
    None) on the positives `pos` [3, B]: the host's lists, the fp64 forward with its two conditions, the exact rows and counts,
    the fp64 update y of the rows whose counts do not cancel and what the rounding hash picks for it."""
    global TRAIN
    if TRAIN is None:
        TRAIN = set(zip(*[a.tolist() for a in graph()]))
    from test_gpu_shared_emit_chunks import forward_chunks
    import shared_in_chunk_ref as icref
    D = full.shape[1]
    K = MODES[mode].get("in_chunk", 0)
    denom = B * (N + K)
    ent_w, rel_w = bf16_ref.widen(full[:E]), bf16_ref.widen(full[E:])
    h, t, r = (pos[i].astype(np.int64) for i in range(3))
    if mode == "position":
        n_chunks = -(-B // P)
        cand = ref.candidates(SHARED_SEED, step, n_chunks, N, E)
        pair = ref.sides(ref.side_draws(SHARED_SEED, step, B, N), r)
        for b in range(B):
            for k in range(N):
                c = int(cand[b // P, k])
                if ((int(h[b]), c, int(r[b])) if pair[b, k] == 0 else (c, int(t[b]), int(r[b]))) in TRAIN:
                    pair[b, k] |= 2
        lists = (cand, pair)
        want = ref.forward(ent_w, rel_w, h, t, r, cand, pair, P, MARGIN, denom)
    else:
        h2, t2, r2, cand, pair, perm, chunks = icref.host_lists(h, t, r, P, E, R, N, K, SHARED_SEED, step, TRAIN, None, type_lists)
        lists = (cand, pair, perm, chunks)
        want = forward_chunks(ent_w, rel_w, h2, t2, r2, cand, pair, chunks, MARGIN, denom)
    rows, counts = ref.reduce(want["keys"], want["records"])
    live = np.abs(counts).sum(1) > 0
    lrows, lcounts = rows[live], counts[live]
    x = bf16_ref.widen(full[lrows])
    y, a1, g = bf16_ref.update(x, lcounts, denom, RATES[opt], None if acc is None else acc[lrows])
    lo, hi = bf16_ref.neighbours(y)
    lo_v, hi_v = np.abs(bf16_ref.widen(lo).astype(np.float64)), np.abs(bf16_ref.widen(hi).astype(np.float64))
    frac = np.where(hi_v > lo_v, (np.abs(y) - lo_v) / np.where(hi_v > lo_v, hi_v - lo_v, 1.0), 0.0)
    rnd = bf16_ref.round_bits(ROUND_SEED, step, lrows.reshape(-1, 1), D, np.arange(D).reshape(1, -1)).astype(np.float64)
    tt = frac * 65536.0 + rnd
    near = np.abs(tt - 65536.0 * np.round(tt / 65536.0)) <= BAND
    pick = np.where(tt >= 65536.0, hi, lo)
    return dict(lists=lists, want=want, rows=rows, counts=counts, live_rows=lrows, y=y, acc=a1, moved=g != 0, lo=lo, hi=hi, near=near,
                pick=pick, stored=bf16_ref.round_rows(y.astype(np.float32), lrows, ROUND_SEED, step), denom=denom)


def check_conditions(want):
    assert want["min_kink"] >= 1e-4, want["min_kink"]
    assert want["min_sign"] >= 1e-5, want["min_sign"]


def apply_by_hand(con, tabs, accs, rows, counts, denom, step):
    """kge_transe_apply_rows_*_bf16 on clones of the pre-step tables with the host's rows and counts."""
    import torch
    from openkeonspark_amd import _lib
    L = con.lib
    tabs = [t.clone() for t in tabs]
    d_rows = torch.from_numpy(rows.astype(np.int32)).cuda()
    d_counts = torch.from_numpy(np.ascontiguousarray(counts.astype(np.int32))).cuda()
    d_n = torch.tensor([len(rows)], dtype=torch.int32, device="cuda")
    seed, st = ctypes.c_uint64(ROUND_SEED), ctypes.c_uint64(step)
    if accs is None:
        _lib.check(L.kge_transe_apply_rows_sgd_bf16(ctypes.byref(con._desc), tabs[0].data_ptr(), tabs[1].data_ptr(), d_rows.data_ptr(),
                                                    d_counts.data_ptr(), d_n.data_ptr(), len(rows), denom, float(con.alpha), seed, st, None), L)
    else:
        accs = [a.clone() for a in accs]
        _lib.check(L.kge_transe_apply_rows_rowadagrad_bf16(ctypes.byref(con._desc), tabs[0].data_ptr(), tabs[1].data_ptr(), accs[0].data_ptr(),
                                                           accs[1].data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), d_n.data_ptr(), len(rows),
                                                           denom, float(con.alpha), seed, st, None), L)
    torch.cuda.synchronize()
    return tabs, accs


def run_three_steps(D, opt, mode, bf16_first=True):
    import torch
    con = make_config(D, opt, mode, bf16_first=bf16_first)
    assert con.sparse_rows and con.use_counts and not con.sparse_inplace and con._bf16 and con._shared_chunk == P
    assert [t.dtype for t in con._tables] == [torch.bfloat16, torch.bfloat16]
    ada = opt == "RowAdagrad"
    typed = mode == "typed_in_chunk"
    type_lists = con.type_constraints() if typed else None
    undecided = moved_n = 0
    for step in range(3):
        tabs = [t.clone() for t in con._tables]
        accs = [a.clone() for a in con._rowadagrad_acc] if ada else None
        full = np.concatenate([bits(t) for t in tabs])
        acc = np.concatenate([a.cpu().numpy() for a in accs]) if ada else None
        # the step's positives, drawn ahead: the sampler's streams are put back
        states = con.get_stream_states()
        dev, n_pos = con._sample_positives()
        pos = dev.cpu().numpy()[:, :B].copy()
        con.lib.kge_set_stream_states(states.ctypes.data, con.workThreads)
        assert n_pos == B
        w = host_step(full, acc, pos, step, mode, opt, type_lists)
        check_conditions(w["want"])                                                    # before the step runs
        share = (w["near"] & w["moved"]).sum() / max(w["moved"].sum(), 1)
        assert share <= 1e-3, share
        loss = con.train_step()
        assert con.global_step == step + 1
        assert np.array_equal(con._sparse_buf["shared_batch"].cpu().numpy()[:, :B], pos)
        for got, want in zip(con.shared_negatives_of(step), w["lists"]):
            assert np.array_equal(got, want)
        print("%s D %d %s step %d: loss %.9g (fp64 %.9g), listed rows %d (%d with counts), min kink %.2e, min sign %.2e, undecided %d of %d"
              % (opt, D, mode, step, loss, w["want"]["loss"], len(w["rows"]), len(w["live_rows"]), w["want"]["min_kink"],
                 w["want"]["min_sign"], int((w["near"] & w["moved"]).sum()), int(w["moved"].sum())))
        assert abs(loss - w["want"]["loss"]) <= 1e-5 * abs(w["want"]["loss"])
        got_full = np.concatenate([bits(t) for t in con._tables])
        rest = np.ones(E + R, bool)
        rest[w["live_rows"]] = False
        assert len(w["live_rows"]) > B and rest.sum() > 0
        np.testing.assert_array_equal(got_full[rest], full[rest])                       # no record, or counts that cancel: every bit stays
        got = got_full[w["live_rows"]]
        assert (got != full[w["live_rows"]]).any()
        assert ((got == w["lo"]) | (got == w["hi"])).all()
        decided = w["moved"] & ~w["near"]
        np.testing.assert_array_equal(got[decided], w["pick"][decided])
        np.testing.assert_array_equal(w["stored"][decided], w["pick"][decided])         # (round_rows of the fp64 y is that pick)
        np.testing.assert_array_equal(got[~w["moved"]], full[w["live_rows"]][~w["moved"]])
        undecided += int((w["near"] & w["moved"]).sum()); moved_n += int(w["moved"].sum())
        if ada:
            got_acc = np.concatenate([a.cpu().numpy() for a in con._rowadagrad_acc])
            np.testing.assert_array_equal(got_acc[rest].view(np.uint32), acc[rest].view(np.uint32))
            assert (np.abs(got_acc[w["live_rows"]].astype(np.float64) - w["acc"]) <= 1e-6 * w["acc"]).all()
        # every element of every row: the apply stage by hand on the host's rows and counts
        hand_tabs, hand_accs = apply_by_hand(con, tabs, accs, w["rows"], w["counts"], w["denom"], step)
        for a, b in zip(con._tables, hand_tabs):
            np.testing.assert_array_equal(bits(a), bits(b))
        if ada:
            for a, b in zip(con._rowadagrad_acc, hand_accs):
                np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    print("%s D %d %s: %d of %d moved elements lie inside the band (left to the neighbour check and the by-hand apply)" % (opt, D, mode, undecided, moved_n))


@pytest.mark.parametrize("opt", ["SGD", "RowAdagrad"])
@pytest.mark.parametrize("D", [8, 200])
def test_three_steps_by_position_equal_the_host_replay(D, opt):
    run_three_steps(D, opt, "position")


@pytest.mark.parametrize("mode", ["relation", "typed_in_chunk"])
@pytest.mark.parametrize("opt", ["SGD", "RowAdagrad"])
@pytest.mark.parametrize("D", [8, 200])
def test_three_steps_on_grouped_chunks_equal_the_host_replay(D, opt, mode):
    run_three_steps(D, opt, mode, bf16_first=False)      # (the setters in the other order)


@pytest.mark.parametrize("mode", ["position", "typed_in_chunk"])
@pytest.mark.parametrize("opt", ["SGD", "RowAdagrad"])
def test_reproducible_and_resumable_bit_for_bit(opt, mode):
    from openkeonspark_amd import distribute_training as dt
    from openkeonspark_amd._lib import KgeError
    D = 8
    whole = make_config(D, opt, mode)
    lw = [whole.train_step() for _ in range(4)]
    again = make_config(D, opt, mode, bf16_first=False)
    la = [again.train_step() for _ in range(2)]
    assert la == lw[:2]
    z = dt.checkpoint_arrays(again)
    assert [int(x) for x in z["table_dtype"]] == [1, ROUND_SEED] and [int(x) for x in z["shared_negatives"]][:2] == [P, SHARED_SEED]
    la += [again.train_step() for _ in range(2)]
    assert la == lw and same(state(again), state(whole))
    resumed = make_config(D, opt, mode, table_seed=2)
    assert dt.restore_checkpoint(resumed, "unused.npz", arrays=dict(z)) == 2
    assert [resumed.train_step() for _ in range(2)] == lw[2:] and same(state(resumed), state(whole))
    for kw, words in ((dict(round_seed=ROUND_SEED + 1), "rounding seed"), (dict(chunk=8), "shared negatives")):
        other = make_config(D, opt, mode, **kw)
        with pytest.raises(KgeError) as e:
            dt.restore_checkpoint(other, "unused.npz", arrays=dict(z))
        assert words in str(e.value)


def test_the_modes_do_not_leak_into_each_other():
    """An fp32 shared run and an unshared bf16 run give the same bits before and after a bf16 + shared run of the process (one
    engine per process: its buffers and options outlive a Config)."""
    D = 8

    def fp32_shared():
        con = make_config(D, "SGD", "relation", bf16=False)
        return [con.train_step() for _ in range(2)], state(con)

    def bf16_unshared():
        con = make_config(D, "RowAdagrad", "position", shared=False)
        return [con.train_step() for _ in range(2)], state(con)

    before = fp32_shared(), bf16_unshared()
    for opt, mode in (("RowAdagrad", "typed_in_chunk"), ("SGD", "position")):
        con = make_config(D, opt, mode)
        for _ in range(2):
            con.train_step()
    after = fp32_shared(), bf16_unshared()
    for (l0, s0), (l1, s1) in zip(before, after):
        assert l0 == l1 and same(s0, s1)
    assert before[0][1][0].dtype == np.uint32 and before[1][1][0].dtype == np.uint16


def test_equal_seeds_are_refused_by_the_session():
    """The rounding hash and the shared-negatives hashes share their step key: one seed for both is refused, two are taken."""
    from openkeonspark_amd._lib import KgeError
    with pytest.raises(KgeError) as e:
        make_config(8, "SGD", "position", round_seed=SHARED_SEED)
    assert "must differ" in str(e.value) and "shared negatives" in str(e.value) and "bf16" in str(e.value)
    con = make_config(8, "SGD", "relation", round_seed=SHARED_SEED + 1)
    assert con._bf16 and con._shared_chunk == P
