"""tests/score_ref.py, checked without a GPU: the fp64 definition against the committed C oracle, the integer scores of the axis
tables against the definition (exactly), and -- for the very seeds the GPU tests use -- the conditions that the fp64 reference
alone must meet for the random comparisons of tests/test_gpu_eval_definition.py to be meaningful."""
import numpy as np
import pytest

import score_ref
from score_ref import MODELS, exact_scores, exact_tables, scores
from oracle import oracle

ORACLE_DIMS = {m: [(7, 7), (100, 100), (260, 260)] for m in ("transe", "transh", "transd")}
ORACLE_DIMS["transr"] = [(7, 12), (100, 64), (260, 33), (33, 260)]


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("model", MODELS)
def test_definition_agrees_with_the_c_oracle(model, scale):
    for De, Dr in ORACLE_DIMS[model]:
        E, R, n = 70, 4, 400
        rng = np.random.default_rng(score_ref.seed_of(model, De, Dr))
        params = {k: (v * scale).astype(np.float32) for k, v in oracle.init_params(oracle.MODEL_IDS[model], E, R, De, Dr, seed=9).items()}
        orc = oracle.Model(model, E, R, De, Dr, params=params)
        h, t, r = rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)
        want = orc.predict(h, t, r).astype(np.float64)               # TransR: the matrix of r[0] for every triple
        got = scores(model, params, h, t, r, De, Dr)
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).min(), (De, Dr)
        if model == "transr":                                        # own_matrix: one oracle call per relation
            got = scores(model, params, h, t, r, De, Dr, "own_matrix")
            assert (got != scores(model, params, h, t, r, De, Dr))[(r != r[0]) & (h != t)].all()      # two contracts, two values
            for q in range(R):
                m = r == q
                assert np.abs(got[m] - orc.predict(h[m], t[m], r[m])).max() <= 1e-5 * got[m].min(), (De, Dr, q)
        # and the fp32 evaluation of the same formula, the yardstick of the GPU reports, is itself far inside 1e-5
        assert score_ref.fp32_error(model, params, h, t, r, De, Dr, got if model == "transr" else want,
                                    "own_matrix" if model == "transr" else "predict") < 1e-5


def all_pairs(E, R, D):
    """Every ordered pair of a set of entities under every relation; at large widths the set is the rows on the special axes
    (every fourth row), a few others and the last rows -- the same properties at a fraction of the fp64 work."""
    if D <= 128:
        ids = np.unique(np.concatenate([np.arange(min(E, 90)), np.arange(max(0, E - 40), E)]))
    else:
        ids = np.unique(np.concatenate([np.arange(3, min(E, 170), 4), np.arange(24), np.arange(E - 10, E)]))
    h, t, r = np.meshgrid(ids, ids, np.arange(R), indexing="ij")
    return h.ravel(), t.ravel(), r.ravel()


@pytest.mark.parametrize("D", [1, 17, 64, 65, 260, 1024])
@pytest.mark.parametrize("model", MODELS)
def test_integer_scores_equal_the_definition_exactly(model, D):
    for De, Dr in ([(D, D)] if model != "transr" else [(D, D), (D, 24), (24, D)]):
        E, R = max(De, 64) + 2, (7 if max(De, Dr) <= 128 else 4)
        params = exact_tables(model, E, R, De, Dr)
        h, t, r = all_pairs(E, R, max(De, Dr))
        for variant in (("predict", "own_matrix") if model == "transr" else ("predict",)):
            want = scores(model, params, h, t, r, De, Dr, variant)
            got = exact_scores(model, params, h, t, r, De, Dr, variant)
            assert got.dtype == np.float32
            if model == "transe":      # the definition's fp64 mean, rounded once, is the one fp32 division of the integer sum
                assert np.array_equal(want.astype(np.float32), got)
                assert np.array_equal(np.rint(want * De), np.rint(got.astype(np.float64) * De))
            else:
                assert np.array_equal(want, got.astype(np.float64))
            assert len(np.unique(got)) >= (3 if De > 1 else 2), "the scores fall into too few classes to tell anything"
        # the fp32 evaluation of the definition gives the same bits: nothing on these tables depends on the precision
        assert np.array_equal(scores(model, params, h, t, r, De, Dr, dtype=np.float32), exact_scores(model, params, h, t, r, De, Dr))


@pytest.mark.parametrize("D", [1, 16, 17, 100, 257, 1024])
def test_axis_tables_reach_the_edges_of_every_rung(D):
    """Rows live on the last element of the row and on both ends of the last slab of the rung (and of every smaller rung)."""
    E = max(D, 64) + 2
    L, C = score_ref.rung_of(D)
    ax = set(score_ref.entity_axes(E, D).tolist())
    assert D - 1 in ax and 0 in ax
    assert min(L * (C - 1), D - 1) in ax
    for top, l, c in score_ref.RUNGS:
        if top < D:
            assert l * c in ax and l * c - 1 in ax           # the first element a rung too small would drop, and the one before it
    for model in MODELS:
        P = exact_tables(model, E, 7, D, D)
        assert (np.abs(P["rel_embeddings"]).argmax(1) == D - 1).any() and not P["rel_embeddings"][0].any()
        if model == "transr":
            M = P["transfer_matrix"].reshape(7, D, D)
            cols = np.abs(M).argmax(-1)
            assert set((cols // 128).ravel().tolist()) == set(range((D + 127) // 128))      # every column block is hit
            assert D < 2 or (cols[:, 1] == cols[:, 0]).all()                               # rows collide on a column


@pytest.mark.parametrize("model,De,Dr", score_ref.EVAL_CASES)
def test_random_cases_meet_the_fp64_conditions(model, De, Dr):
    """At most 5 % of the rank queries have a candidate within 2e-5 of the target, and at most 5 % of the top-k queries have
    their k-th and (k+1)-th scores that close: asserted here so that a bad seed is found without a GPU."""
    case = score_ref.eval_case(model, De, Dr, "random")
    ev = case["ev"]
    h, t, r = score_ref.eval_queries(case["graph"])
    counts, aside = ev.rank_counts(h, t, r, score_ref.BAND)
    assert aside.mean() <= score_ref.MAX_ASIDE and counts[:, :, 0].any()
    assert (counts[:, :, 1] < counts[:, :, 0]).any() and (counts[:, :, 2] < counts[:, :, 0]).any()
    th, tt, tr = case["graph"]["test"]                        # link_prediction and relation_prediction rank the test split alone
    assert ev.rank_counts(th, tt, tr, score_ref.BAND)[1].mean() <= score_ref.MAX_ASIDE
    rel_counts, rel_aside = ev.relation_counts(th, tt, tr, score_ref.BAND)
    assert rel_aside.mean() <= score_ref.MAX_ASIDE and rel_counts[:, 0].any()
    for k in score_ref.RANDOM_K:
        for head in (False, True):
            for filtered in (False, True):
                assert ev.top_k_entities(t if head else h, r, head, k, filtered, score_ref.BAND)[2].mean() <= score_ref.MAX_ASIDE
    for k in score_ref.RANDOM_K_REL:
        for filtered in (False, True):
            assert ev.top_k_relations(h, t, k, filtered, score_ref.BAND)[2].mean() <= score_ref.MAX_ASIDE


def test_exact_cases_have_ties_and_every_filter_bites():
    case = score_ref.eval_case("transe", 64, 64, "exact")
    h, t, r = score_ref.eval_queries(case["graph"])
    counts, _ = case["ev"].rank_counts(h, t, r)
    assert (counts[:, :, 1] < counts[:, :, 0]).any() and (counts[:, :, 2] < counts[:, :, 0]).any() and (counts[:, :, 3] < counts[:, :, 2]).any()
    s = case["ev"].entity_scores(h[0], r[0], False)[0]
    assert len(np.unique(s)) <= 4 and np.bincount((s * 64).astype(np.int64)).max() > 50        # a few classes, massive ties
