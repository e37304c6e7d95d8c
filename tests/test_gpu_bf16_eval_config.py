"""Config on bf16 tables: the evaluators that only gather rows -- test_step, triple classification, rank_candidates,
rank_triples_sampled, validation_link_prediction(candidates=C) -- read the stored rows (kge_predict_bf16,
kge_rank_candidates_bf16): the results of an fp32 Config holding the widened parameters, no float32 view, the tables untouched.
The full-entity evaluators still make the view and a training step still drops it.  Then the point of it in bytes: ranking
against drawn candidates on a 262 144 x 64 table allocates less than half a view, rank_triples at least a whole one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, R, B, N_NEG, N_BATCHES, D = 500, 7, 301, 5, 4, 24
SEED = 0xB16B00B5


def triples(ent=E, n_train=B * N_BATCHES, n_eval=40):
    rng = np.random.default_rng(99)
    seen = set()
    while len(seen) < n_train + 2 * n_eval:
        h = int(rng.integers(0, ent)); t = int((h + 1 + rng.integers(0, ent - 1)) % ent)
        seen.add((h, t, int(rng.integers(0, R))))
    a = np.array(sorted(seen), np.int64)
    rng.shuffle(a)
    return a[:n_train], a[n_train:n_train + n_eval], a[n_train + n_eval:]


def engine(dtype, ent=E, dim=D, splits=None):
    import openkeonspark_amd as pkg
    train, valid, test = splits if splits is not None else triples()
    con = pkg.Config()
    con.set_work_threads(4)
    con.set_ent_neg_rate(N_NEG); con.set_rel_neg_rate(0); con.set_margin(1.0)
    con.set_opt_method("SGD"); con.set_alpha(0.5)
    con.set_dimension(dim)
    con.set_nbatches(N_BATCHES)
    con.seed = 3
    if dtype is not None:
        con.set_table_dtype(dtype, seed=SEED)
    con.init_from_arrays(ent, R, train[:, 0], train[:, 1], train[:, 2])
    con.init_evaluation_from_arrays(tuple(valid.T), tuple(test.T), derive_types=True)
    con.set_model_and_session(pkg.TransE)
    return con


def bits(con):
    import torch
    return [t.detach().view(torch.int16).cpu().numpy().copy() for t in con._tables]


def same(a, b):
    """Arrays bit for bit, everything else ==, through tuples and dicts."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def test_row_gathering_evaluators_read_the_bf16_tables_and_make_no_view():
    con = engine("bf16")
    assert con._tables[0].element_size() == 2
    for _ in range(2):
        con.train_step()
    fp32 = engine(None)
    fp32.set_parameters(con.get_parameters())
    _, _, test = triples()
    h, t, r = test[:, 0], test[:, 1], test[:, 2]
    rng = np.random.default_rng(5)
    tails, heads = rng.integers(-1, E + 2, (len(h), 19)), rng.integers(-1, E + 2, (len(h), 19))
    tails[::2, 3], heads[::2, 4] = t[::2], h[::2]
    restart = lambda c: c.lib.kge_set_option(b"libc_rand_restart", 1)      # triple classification draws its negatives with rand()
    ops = {
        "test_step": lambda c: c.test_step(h, t, r),
        "rank_candidates": lambda c: c.rank_candidates(h, t, r, tails, heads),
        "rank_candidates, one shared list, unfiltered": lambda c: c.rank_candidates(h, t, r, tails[0], None, filtered=False),
        "rank_triples_sampled": lambda c: c.rank_triples_sampled(h, t, r, 16, seed=11),
        "rank_triples_sampled, typed": lambda c: c.rank_triples_sampled(h, t, r, 16, seed=11, type_constrained=True),
        "validation_link_prediction(candidates=16)": lambda c: c.validation_link_prediction(candidates=16, seed=3),
        "validation_accuracy": lambda c: (restart(c), c.validation_accuracy())[1],
        "triple_classification": lambda c: (restart(c), c.triple_classification())[1],
        "roc_auc": lambda c: (restart(c), c.roc_auc("valid"))[1],
    }
    before = bits(con)
    assert con._eval_view is None
    for name, op in ops.items():
        got, want = op(con), op(fp32)
        if name == "roc_auc":      # (NaN for a relation without triples in the split: compare the bits)
            got, want = {k: np.asarray(v) for k, v in got.items()}, {k: np.asarray(v) for k, v in want.items()}
        assert same(got, want), (name, got, want)
        assert con._eval_view is None, name
        assert same(bits(con), before), name
    counts, metrics = ops["rank_triples_sampled"](con)
    assert counts[:, :, 0].any() and 0.0 < metrics["r_filter_reci_rank"] <= 1.0
    assert ops["triple_classification"](con)["tp"] > 0
    # the full-entity evaluators still read a float32 view, and the next training step drops it
    got, want = con.rank_triples(h, t, r), fp32.rank_triples(h, t, r)
    assert same(got, want)
    assert con._eval_view is not None and con._eval_view[0][0].element_size() == 4
    ops["test_step"](con)
    ops["rank_triples_sampled"](con)
    assert con._eval_view is not None          # ... which the direct readers neither need nor disturb
    con.train_step()
    assert con._eval_view is None


def test_ranking_against_drawn_candidates_allocates_no_table_sized_buffer():
    import torch
    ent, dim, n, C = 262144, 64, 100, 64
    splits = triples(ent, n_train=B * N_BATCHES, n_eval=n)
    con = engine("bf16", ent=ent, dim=dim, splits=splits)
    view_bytes = sum(t.numel() for t in con._tables) * 4
    assert view_bytes >= 67_000_000
    h, t, r = splits[2][:, 0], splits[2][:, 1], splits[2][:, 2]
    assert len(h) == n

    def peak_rise(op):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = op()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    rise, (counts, _) = peak_rise(lambda: con.rank_triples_sampled(h, t, r, C, seed=1))
    print("rank_triples_sampled: peak rise %d bytes; a float32 view is %d" % (rise, view_bytes))
    assert counts.shape == (n, 2, 2) and counts[:, :, 0].any()
    assert rise < view_bytes // 2 and con._eval_view is None
    rise, _ = peak_rise(lambda: con.test_step(h, t, r))
    assert rise < view_bytes // 2 and con._eval_view is None
    rise, _ = peak_rise(lambda: con.rank_triples(h[:4], t[:4], r[:4]))
    print("rank_triples: peak rise %d bytes" % rise)
    assert rise >= view_bytes and con._eval_view is not None          # the control: the measure sees a view when one is made
