"""The host half of candidate-list ranking (Config.rank_candidates / rank_triples_sampled): the numpy restatement of the device's
counter hash against the formula of include/kge_mi355.h written out with Python integers, the metric names and values from a
hand-made count array, and the driver's new options.  No GPU and no engine: the Config methods are called on a stand-in."""
import types

import numpy as np
import pytest

from openkeonspark_amd import _lib, rank_eval
from openkeonspark_amd import distribute_training as dt
from openkeonspark_amd.Config import Config

M64 = (1 << 64) - 1


def formula(seed, i, s, k, length):
    """include/kge_mi355.h, KGE_RANKC_DRAWN, in unbounded Python integers reduced mod 2^64."""
    c = ((2 * i + s) << 32) | k
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * length) >> 32


def stand_in(E, lists=None):
    """What sampled_candidates reads of a Config: entTotal and type_constraints()."""
    con = types.SimpleNamespace(entTotal=E)
    con.type_constraints = lambda: lists
    return con


@pytest.mark.parametrize("E", [1, 7, 300, 2 ** 31 - 1])
@pytest.mark.parametrize("seed", [0, 12345, 2 ** 64 - 1])
def test_sampled_candidates_is_the_formula(E, seed):
    n, C = 9, 33
    for side in (0, 1):
        got = Config.sampled_candidates(stand_in(E), n, C, seed, side)
        assert got.dtype == np.int64 and got.shape == (n, C)
        want = np.array([[formula(seed, i, side, k, E) for k in range(C)] for i in range(n)])
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < E
    if E >= 300:      # the two sides and two seeds draw different lists
        assert not np.array_equal(Config.sampled_candidates(stand_in(E), n, C, seed, 0), Config.sampled_candidates(stand_in(E), n, C, seed, 1))
        assert not np.array_equal(Config.sampled_candidates(stand_in(E), n, C, seed, 0), Config.sampled_candidates(stand_in(E), n, C, seed ^ 1, 0))


def test_large_triple_and_candidate_indices():
    """The counter packs (2 i + s) above bit 32: indices near the entry point's limits (n < 2^30, k < 2^31) stay exact."""
    i = np.array([0, 1, 2 ** 30 - 1]); k = np.array([0, 2 ** 31 - 1, 77])
    got = _lib.drawn_candidate_index(99, i[:, None], 1, k[None, :], 2 ** 31 - 1)
    want = np.array([[formula(99, int(a), 1, int(b), 2 ** 31 - 1) for b in k] for a in i])
    assert np.array_equal(got, want)


def test_uniform_over_the_entities():
    ids = Config.sampled_candidates(stand_in(7), 2000, 50, 3, 0)
    share = np.bincount(ids.reshape(-1), minlength=7) / ids.size
    assert np.abs(share - 1 / 7).max() < 0.01          # 10^5 draws: a standard deviation of 0.0011 per cell


def test_typed_draws_index_the_relations_list_and_fall_back_when_it_is_empty():
    E, R = 300, 4
    rng = np.random.default_rng(2)
    head = [np.sort(rng.choice(E, 40, replace=False)), np.zeros(0, np.int64), np.arange(5), np.sort(rng.choice(E, 170, replace=False))]
    tail = [np.arange(E - 3, E), np.zeros(0, np.int64), np.sort(rng.choice(E, 99, replace=False)), np.array([7])]
    csr = lambda ls: (np.cumsum([0] + [len(x) for x in ls]).astype(np.int64), np.concatenate(ls).astype(np.int64))
    lists = csr(head) + csr(tail)
    r = np.array([0, 1, 2, 3, 3, 1, 0])
    for side, ls in ((0, tail), (1, head)):
        got = Config.sampled_candidates(stand_in(E, lists), len(r), 21, 5, side, r=r, type_constrained=True)
        for i, q in enumerate(r.tolist()):
            for k in range(21):
                want = formula(5, i, side, k, E) if len(ls[q]) == 0 else ls[q][formula(5, i, side, k, len(ls[q]))]
                assert got[i, k] == want, (side, i, k)
    untyped = Config.sampled_candidates(stand_in(E, lists), len(r), 21, 5, 0)
    typed = Config.sampled_candidates(stand_in(E, lists), len(r), 21, 5, 0, r=r, type_constrained=True)
    assert np.array_equal(typed[1], untyped[1]) and np.array_equal(typed[5], untyped[5]) and not np.array_equal(typed[0], untyped[0])
    with pytest.raises(Exception):
        Config.sampled_candidates(stand_in(E, lists), len(r), 21, 5, 0, type_constrained=True)          # no relations given
    # all lists empty: every draw is untyped
    empty = (np.zeros(R + 1, np.int64), np.zeros(0, np.int64)) * 2
    assert np.array_equal(Config.sampled_candidates(stand_in(E, empty), len(r), 21, 5, 1, r=r, type_constrained=True),
                          Config.sampled_candidates(stand_in(E), len(r), 21, 5, 1))


def test_metric_names_and_values_from_hand_made_counts():
    counts = np.zeros((4, 2, 2), np.int64)
    counts[:, 0, 0] = [0, 2, 9, 10]          # tail side, raw
    counts[:, 0, 1] = [0, 0, 3, 9]           # tail side, filtered
    counts[:, 1, 0] = [1, 1, 1, 100]
    counts[:, 1, 1] = [0, 1, 1, 50]
    m = rank_eval.normalise(rank_eval.cand_sums(counts), 4)
    names = {p + mid + end for p in "rl" for mid in ("", "_filter") for end in ("_tot", "_rank", "_reci_rank")} | \
            {p + k + mid + "_tot" for p in "rl" for k in "31" for mid in ("", "_filter")}
    assert set(m) == names and not any("constrain" in k for k in m)
    assert m["r_tot"] == 0.75 and m["r3_tot"] == 0.5 and m["r1_tot"] == 0.25
    assert m["r_filter_tot"] == 1.0 and m["r3_filter_tot"] == 0.5 and m["r1_filter_tot"] == 0.5
    assert m["r_rank"] == (1 + 3 + 10 + 11) / 4 and m["r_filter_rank"] == (1 + 1 + 4 + 10) / 4
    assert m["r_reci_rank"] == pytest.approx((1 + 1 / 3 + 1 / 10 + 1 / 11) / 4, rel=1e-15)
    assert m["l_tot"] == 0.75 and m["l1_tot"] == 0.0 and m["l1_filter_tot"] == 0.25
    assert m["l_filter_reci_rank"] == pytest.approx((1 + 0.5 + 0.5 + 1 / 51) / 4, rel=1e-15)
    tail_only = rank_eval.cand_sums(counts, (0,))
    assert tail_only and all(k.startswith("r") for k in tail_only)
    # link_prediction's own sums keep their forty names and values
    out = np.zeros((4, 2, 8), np.int64)
    out[:, :, 0], out[:, :, 1] = counts[:, :, 0], counts[:, :, 1]
    lp = rank_eval.normalise(rank_eval.lp_sums(out), 4)
    assert len(lp) == 40 and all(lp[k] == m[k] for k in m)
    assert lp["r_tot_constrain"] == 1.0 and lp["l_filter_reci_rank_constrain"] == 1.0


def test_a_sharded_entity_table_is_refused_before_anything_else():
    """Every entrance refuses a row-sharded entity table first: the stand-in has nothing else a call could go on with."""
    from openkeonspark_amd.Config import KgeError
    con = types.SimpleNamespace(_sharded=lambda name: name == "ent_embeddings", world_size=2)
    con._refuse_sharded_candidates = types.MethodType(Config._refuse_sharded_candidates, con)
    for call in (lambda: Config.rank_candidates(con, [0], [1], [0], [2, 3]), lambda: Config.rank_triples_sampled(con, [0], [1], [0], 5),
                 lambda: Config.rank_triples_sampled_distributed(con, [0], [1], [0], 5),
                 lambda: Config.validation_link_prediction(con, candidates=5)):
        with pytest.raises(KgeError, match="sharded across ranks"):
            call()
    replicated = types.SimpleNamespace(_sharded=lambda name: False)
    Config._refuse_sharded_candidates(replicated, "rank_candidates")          # no exception


def test_the_driver_options_default_to_ranking_every_entity(capsys):
    args = dt.parse_args([])
    assert args.early_stop_candidates == 0 and args.early_stop_candidates_seed == 0
    args = dt.parse_args(["--early_stop_metric", "mrr", "--early_stop_candidates", "500", "--early_stop_candidates_seed", "7"])
    assert args.early_stop_candidates == 500 and args.early_stop_candidates_seed == 7
    with pytest.raises(SystemExit):
        dt.parse_args(["--help"])
    helptext = " ".join(capsys.readouterr().out.split())
    assert helptext.count("--early_stop_candidates") >= 3          # the usage line, its own entry, the mention in --early_stop_metric's help
