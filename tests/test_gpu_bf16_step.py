"""bf16 table storage through Config (set_table_dtype("bf16")): E = 500, R = 7, B = 301, n = 5, widths 24 and 200, SGD and
RowAdagrad.  The tables are torch.bfloat16 and half the bytes; train_step equals the stages called by hand (emit, reduce, apply
with the same seed and step) bit for bit, and a second run equals the first; the loss is the fp32 emit's on the widened tables;
a checkpoint resumes bit for bit; parameters round-trip; the evaluation calls equal an fp32 Config's on the widened parameters;
the refusals that need a Config are raised with their reasons."""
import ctypes

import numpy as np
import pytest

import bf16_ref as ref

pytestmark = pytest.mark.gpu

E, R, B, N_NEG, N_BATCHES = 500, 7, 301, 5, 4
SEED = 0xB16B00B5


def triples():
    rng = np.random.default_rng(99)
    seen = set()
    while len(seen) < B * N_BATCHES + 80:
        h = int(rng.integers(0, E)); t = int((h + 1 + rng.integers(0, E - 1)) % E)
        seen.add((h, t, int(rng.integers(0, R))))
    a = np.array(sorted(seen), np.int64)
    rng.shuffle(a)
    return a[:B * N_BATCHES], a[B * N_BATCHES:B * N_BATCHES + 40], a[B * N_BATCHES + 40:]


def engine(D, opt, dtype="bf16", streams=None, model="TransE", evaluation=False, **kw):
    import openkeonspark_amd as pkg
    train, valid, test = triples()
    con = pkg.Config()
    con.set_work_threads(4)
    con.set_ent_neg_rate(kw.pop("n_ent", N_NEG)); con.set_rel_neg_rate(0); con.set_margin(1.0)
    con.set_opt_method(opt); con.set_alpha(0.5 if opt == "SGD" else 0.05)
    con.set_dimension(D)
    con.set_nbatches(N_BATCHES)
    con.seed = 3
    for k, v in kw.items():
        setattr(con, k, v)
    if dtype is not None:
        con.set_table_dtype(dtype, seed=SEED)
    con.init_from_arrays(E, R, train[:, 0], train[:, 1], train[:, 2])
    if evaluation:
        con.init_evaluation_from_arrays(tuple(valid.T), tuple(test.T))
    assert con.batch_size == B
    con.set_model_and_session(getattr(pkg, model))
    if streams is not None:
        con.lib.kge_set_stream_states(np.ascontiguousarray(streams, np.uint64).ctypes.data, con.workThreads)
    return con


def bits(t):
    import torch
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16)


def hand_step(con, tabs, accs, dev, n_pos, step):
    """emit -> reduce -> apply by hand on the bf16 tensors `tabs` (and accumulators `accs`) -> the loss."""
    import torch
    from openkeonspark_amd import _lib
    L = con.lib
    n_neg, D = N_NEG, con.hidden_size
    stride = dev.shape[1] // (1 + n_neg)
    M = stride * (3 + n_neg)
    dw = int(L.kge_transe_record_dwords(ctypes.byref(con._desc)))
    rec = torch.empty((M, dw), dtype=torch.int32, device="cuda")
    dst = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    rows = torch.empty(M, dtype=torch.int32, device="cuda")
    counts = torch.empty((M, D), dtype=torch.int32, device="cuda")
    n_rows = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    denom = B * n_neg
    _lib.check(L.kge_transe_emit_records_bf16(ctypes.byref(con._desc), tabs[0].data_ptr(), tabs[1].data_ptr(), dev[0].data_ptr(),
                                              dev[1].data_ptr(), dev[2].data_ptr(), n_pos, n_neg, stride, denom, rec.data_ptr(),
                                              dst.data_ptr(), loss.data_ptr(), None), L)
    # the fp32 emit on the widened tables: the loss train_step must report
    f = [t.float() for t in tabs]
    L.kge_set_option(b"tables_changed", 1)      # fresh fp32 tensors may reuse an address whose 1/|row| table the engine still holds
    rec32, dst32, loss32 = torch.empty_like(rec), torch.full_like(dst, -1), torch.zeros(1, device="cuda")
    _lib.check(L.kge_transe_emit_records(ctypes.byref(con._desc), f[0].data_ptr(), f[1].data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(),
                                         dev[2].data_ptr(), n_pos, n_neg, stride, denom, rec32.data_ptr(), dst32.data_ptr(), None, None,
                                         loss32.data_ptr(), None), L)
    _lib.check(L.kge_transe_reduce_records(ctypes.byref(con._desc), rec.data_ptr(), dst.data_ptr(), M, rows.data_ptr(), counts.data_ptr(),
                                           n_rows.data_ptr(), None), L)
    seed, st = ctypes.c_uint64(SEED), ctypes.c_uint64(step)
    if accs is None:
        _lib.check(L.kge_transe_apply_rows_sgd_bf16(ctypes.byref(con._desc), tabs[0].data_ptr(), tabs[1].data_ptr(), rows.data_ptr(),
                                                    counts.data_ptr(), n_rows.data_ptr(), M, denom, float(con.alpha), seed, st, None), L)
    else:
        _lib.check(L.kge_transe_apply_rows_rowadagrad_bf16(ctypes.byref(con._desc), tabs[0].data_ptr(), tabs[1].data_ptr(),
                                                           accs[0].data_ptr(), accs[1].data_ptr(), rows.data_ptr(), counts.data_ptr(),
                                                           n_rows.data_ptr(), M, denom, float(con.alpha), seed, st, None), L)
    torch.cuda.synchronize()
    return float(loss.item()), float(loss32.item())


@pytest.mark.parametrize("opt", ["SGD", "RowAdagrad"])
@pytest.mark.parametrize("D", [24, 200])
def test_train_step_is_the_stages_by_hand_and_repeats(D, opt):
    import torch
    con = engine(D, opt)
    assert con.sparse_rows and con.use_counts and not con.sparse_inplace and not con.prefetch_sampling
    assert [t.dtype for t in con._tables] == [torch.bfloat16, torch.bfloat16]
    assert [t.numel() * t.element_size() for t in con._tables] == [E * D * 2, R * D * 2]
    ada = opt == "RowAdagrad"
    start = con.get_stream_states()
    first = []
    for step in range(3):
        states = con.get_stream_states()
        tabs = [t.clone() for t in con._tables]
        accs = [a.clone() for a in con._rowadagrad_acc] if ada else None
        assert con.global_step == step
        loss = con.train_step()
        assert (bits(con._tables[0]) != bits(tabs[0])).any() and con.global_step == step + 1
        con.lib.kge_set_stream_states(states.ctypes.data, con.workThreads)      # draw that batch again
        dev, n_pos = con.sample_device()
        by_hand, fp32_loss = hand_step(con, tabs, accs, dev.clone(), n_pos, step)
        assert loss == by_hand
        print("step %d loss %.9g fp32 emit %.9g" % (step, loss, fp32_loss))
        assert abs(loss - fp32_loss) <= 1e-5 * abs(fp32_loss)
        for got, want in zip(con._tables, tabs):
            np.testing.assert_array_equal(bits(got), bits(want))
        if ada:
            for got, want in zip(con._rowadagrad_acc, accs):
                np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
        first.append((loss, [bits(t) for t in con._tables], [a.cpu().numpy() for a in con._rowadagrad_acc] if ada else []))
    again = engine(D, opt, streams=start)
    for step in range(3):
        assert again.train_step() == first[step][0]
    for got, want in zip(again._tables, first[-1][1]):
        np.testing.assert_array_equal(bits(got), want)
    if ada:
        for got, want in zip(again._rowadagrad_acc, first[-1][2]):
            np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("opt", ["SGD", "RowAdagrad"])
def test_two_steps_save_restore_two_steps_is_four_steps(opt):
    from openkeonspark_amd import distribute_training as dt
    from openkeonspark_amd._lib import KgeError
    D = 24
    whole = engine(D, opt)
    start = whole.get_stream_states()
    for _ in range(4):
        whole.train_step()
    half = engine(D, opt, streams=start)
    for _ in range(2):
        half.train_step()
    z = dt.checkpoint_arrays(half)
    assert [int(x) for x in z["table_dtype"]] == [1, SEED] and z["ent_embeddings"].dtype == np.float32
    np.testing.assert_array_equal(ref.to_bf16(z["ent_embeddings"]), bits(half._tables[0]))      # float32, an exact widening
    if opt == "RowAdagrad":
        assert z["ent_embeddings/RowAdagrad"].shape == (E,)
    resumed = engine(D, opt)
    assert dt.restore_checkpoint(resumed, "unused.npz", arrays=dict(z)) == 2
    for _ in range(2):
        resumed.train_step()
    for got, want in zip(resumed._tables, whole._tables):
        np.testing.assert_array_equal(bits(got), bits(want))
    if opt == "RowAdagrad":
        for got, want in zip(resumed._rowadagrad_acc, whole._rowadagrad_acc):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    # another rounding seed is refused; an fp32 run takes the bf16 checkpoint; a bf16 run takes an fp32 checkpoint, rounded once
    other = engine(D, opt)
    other.set_table_dtype("bf16", seed=SEED + 1)
    with pytest.raises(KgeError) as e:
        dt.restore_checkpoint(other, "unused.npz", arrays=dict(z))
    assert "rounding seed" in str(e.value)
    fp32 = engine(D, opt, dtype=None)
    assert dt.restore_checkpoint(fp32, "unused.npz", arrays=dict(z)) == 2
    np.testing.assert_array_equal(fp32.get_parameters()["ent_embeddings"], z["ent_embeddings"])
    z32 = dt.checkpoint_arrays(fp32)
    assert "table_dtype" not in z32
    z32["ent_embeddings"] = (z32["ent_embeddings"] * np.float32(1.001)).astype(np.float32)      # off the bf16 grid
    back = engine(D, opt)
    assert dt.restore_checkpoint(back, "unused.npz", arrays=dict(z32)) == 2
    np.testing.assert_array_equal(bits(back._tables[0]), ref.to_bf16(z32["ent_embeddings"]))


def test_parameters_round_trip_and_creation_rounds_the_fp32_draw():
    D = 24
    con = engine(D, "SGD")
    fp32 = engine(D, "SGD", dtype=None)
    for name, t in zip(con.trainModel.table_names, con._tables):
        np.testing.assert_array_equal(bits(t), ref.to_bf16(fp32.get_parameters()[name]))      # drawn as the fp32 run draws, rounded
    con.train_step()
    p = con.get_parameters()
    assert all(v.dtype == np.float32 for v in p.values())
    before = [bits(t).copy() for t in con._tables]
    con.set_parameters(p)
    for t, want in zip(con._tables, before):
        np.testing.assert_array_equal(bits(t), want)
    np.testing.assert_array_equal(ref.widen(before[0]), p["ent_embeddings"])
    off = {k: (v * np.float32(1.003)).astype(np.float32) for k, v in p.items()}
    con.set_parameters(off)
    np.testing.assert_array_equal(bits(con._tables[0]), ref.to_bf16(off["ent_embeddings"]))      # nearest-even


def test_evaluation_reads_a_float32_view_that_the_next_step_drops():
    D = 24
    con = engine(D, "SGD", evaluation=True)
    for _ in range(2):
        con.train_step()
    params = con.get_parameters()
    _, _, test = triples()
    h, t, r = test[:, 0], test[:, 1], test[:, 2]
    assert con._eval_view is None
    got = (con.test_step(h, t, r), con.rank_triples(h, t, r), con.link_prediction())
    assert con._eval_view is not None and con._eval_view[0][0].dtype.is_floating_point and con._eval_view[0][0].element_size() == 4
    view_ptr = con._eval_view[0][0].data_ptr()
    con.test_step(h, t, r)
    assert con._eval_view[0][0].data_ptr() == view_ptr      # cached
    fp32 = engine(D, "SGD", dtype=None, evaluation=True)
    fp32.set_parameters(params)
    want = (fp32.test_step(h, t, r), fp32.rank_triples(h, t, r), fp32.link_prediction())
    np.testing.assert_array_equal(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(g[0], w[0])
        assert g[1] == w[1]
    con.get_parameters()
    assert con._eval_view is not None
    con.train_step()
    assert con._eval_view is None
    con.test_step(h, t, r)
    con.set_parameters(params)
    assert con._eval_view is None


@pytest.mark.parametrize("kw,reason", [
    (dict(model="TransH"), "built for TransE only"),
    (dict(opt="LazyAdam"), "needs SGD or RowAdagrad"),
    (dict(opt="Adagrad"), "needs SGD or RowAdagrad"),
    (dict(D=100), "multiple of 8"),
    (dict(use_counts=False), "sign-count path"),
    (dict(n_ent=70), "sign-count path"),
])
def test_set_model_and_session_refuses_with_the_reason(kw, reason):
    from openkeonspark_amd._lib import KgeError
    kw = dict(kw)
    with pytest.raises(KgeError) as e:
        engine(kw.pop("D", 24), kw.pop("opt", "SGD"), **kw)
    assert reason in str(e.value) and "bf16" in str(e.value)


def test_shared_negatives_the_persistent_launch_and_ranks_are_refused():
    import openkeonspark_amd as pkg
    from openkeonspark_amd._lib import KgeError
    train, _, _ = triples()
    con = pkg.Config()
    con.set_work_threads(4); con.set_ent_neg_rate(N_NEG); con.set_dimension(24); con.set_nbatches(N_BATCHES)
    con.set_table_dtype("bf16")
    con.set_shared_negatives(8)
    con.init_from_arrays(E, R, train[:, 0], train[:, 1], train[:, 2])
    with pytest.raises(KgeError) as e:
        con.set_model_and_session(pkg.TransE)
    assert "shared negatives" in str(e.value) and "bf16" in str(e.value)
    con = engine(24, "SGD")
    with pytest.raises(KgeError) as e:
        con.train_steps(2, persistent=True)
    assert "persistent" in str(e.value) and "bf16" in str(e.value)
    assert len(con.train_steps(2)) == 2 and con.global_step == 2      # (the plain loop of train_step is not the persistent launch)
    con.force_data_parallel = True      # more than one rank, or its one-rank rehearsal
    with pytest.raises(KgeError) as e:
        con.train_step()
    assert "single-process only" in str(e.value)
    ranks = engine(24, "SGD")
    ranks.world_size = 2      # what init_distributed learns from the process group
    with pytest.raises(KgeError) as e:
        ranks._setup_partition()
    assert "single-process only" in str(e.value) and "bf16" in str(e.value)
    with pytest.raises(KgeError):
        con.set_table_dtype("fp16")
    with pytest.raises(KgeError):
        pkg.Config().set_table_dtype("bf16", seed=-1)
