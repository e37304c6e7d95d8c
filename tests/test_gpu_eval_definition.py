"""The fused evaluators against the score's DEFINITION (tests/score_ref.py), not against kge_predict: rank_triples,
link_prediction, top_k_tails / top_k_heads, top_k_relations, relation_prediction and triple_classification at one width per
rung of the team-shape ladder, for all four models (TransR by each relation's own matrix).

On the axis tables the scores are small integers with massive ties, so every expected count, id and padding position is a
plain integer from exact_scores, a Python set of the known triples and the type lists, with no tolerance.  On random tables
the fp64 scores decide: a query is set aside only when fp64 itself cannot tell (a candidate within 2e-5 of the target, or of
the k-th score), which tests/test_score_ref.py holds under 5 % of the queries for these very seeds."""
import numpy as np
import pytest

import score_ref
from conftest import parity_report
from gpu_engine import make_engine
from score_ref import BAND, EVAL_CASES, MAX_ASIDE, Evaluators, exact_scores, scores

pytestmark = pytest.mark.gpu

RTOL = 1e-5
K_EXACT = (1, 10, 1024)          # 1024: the largest k the entry points take, more than there are candidates


def engine_for(case, model, De, Dr, lists=None, derive=False):
    g = case["graph"]
    con = make_engine(model, g["E"], g["R"], De, Dr, case["params"], train=g["train"])
    con.init_evaluation_from_arrays(g["valid"], g["test"], type_lists=None if derive else lists, derive_types=derive)
    return con


def lp_order(test):
    """The test triples in link_prediction's order: sorted by (r, h, t)."""
    h, t, r = test
    o = np.lexsort((t, h, r))
    return h[o], t[o], r[o]


def same_bits(got, want):
    """The header promises the top-k scores only up to the contraction of kge_predict's products, but on the axis tables every
    product and sum is exact, so there is nothing to contract: the returned scores are exact_scores' bits, padding +inf."""
    return got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.asarray(want, np.float32).view(np.uint32))


@pytest.mark.parametrize("model,De,Dr,types", [c + ("lists",) for c in EVAL_CASES] + [("transe", 64, 64, "derived"), ("transr", 33, 50, "derived")])
def test_axis_tables_every_evaluator_exactly(model, De, Dr, types):
    case = score_ref.eval_case(model, De, Dr, "exact")
    g = case["graph"]
    lists = score_ref.derived_type_lists(g) if types == "derived" else case["lists"]
    ev = Evaluators(case["score"], g, lists)
    con = engine_for(case, model, De, Dr, lists, derive=types == "derived")
    if types == "derived":
        for got, want in zip(con.type_constraints(), lists):
            assert np.array_equal(got, want)
    h, t, r = score_ref.eval_queries(g)

    want, _ = ev.rank_counts(h, t, r)
    assert (want[:, :, 1] < want[:, :, 0]).any() and (want[:, :, 2] < want[:, :, 0]).any() and (want[:, :, 3] < want[:, :, 2]).any()
    got, _ = con.rank_triples(h, t, r)
    assert np.array_equal(got, want), ("rank_triples", np.argwhere(got != want)[:5].tolist())
    th, tt, tr = lp_order(g["test"])
    got = con.link_prediction()[0][:, :, :4]
    assert np.array_equal(got, ev.rank_counts(th, tt, tr)[0]), "link_prediction"

    for k in K_EXACT:
        for filtered in (False, True):
            for head, fixed, call in ((False, h, con.top_k_tails), (True, t, con.top_k_heads)):
                want_ids, want_s, _ = ev.top_k_entities(fixed, r, head, k, filtered)
                ids, sc = call(fixed, r, k, filtered=filtered)
                assert np.array_equal(ids, want_ids), ("top-k entities", k, filtered, head, np.argwhere(ids != want_ids)[:5].tolist())
                assert same_bits(sc, want_s), ("top-k entity scores", k, filtered, head)
            want_ids, want_s, _ = ev.top_k_relations(h, t, k, filtered)
            ids, sc = con.top_k_relations(h, t, k, filtered=filtered)
            assert np.array_equal(ids, want_ids), ("top-k relations", k, filtered, np.argwhere(ids != want_ids)[:5].tolist())
            assert same_bits(sc, want_s), ("top-k relation scores", k, filtered)
    assert (want_ids == -1).any()                      # fewer than k eligible: padded

    want, _ = ev.relation_counts(th, tt, tr)
    got = con.relation_prediction()[0]
    assert np.array_equal(got, want), ("relation_prediction", np.argwhere(got != want)[:5].tolist())
    assert want[:, 0].any() and (want[:, 1] < want[:, 0]).any()


@pytest.mark.parametrize("model,De,Dr", EVAL_CASES)
def test_random_tables_agree_with_fp64_wherever_fp64_can_tell(model, De, Dr):
    case = score_ref.eval_case(model, De, Dr, "random")
    g, ev = case["graph"], case["ev"]
    con = engine_for(case, model, De, Dr, case["lists"])
    h, t, r = score_ref.eval_queries(g)
    shares = {}

    def counts_agree(name, got, want, aside):
        shares[name] = float(aside.mean())
        assert aside.mean() <= MAX_ASIDE, (name, aside.mean())
        assert np.array_equal(got[~aside], want[~aside]), (name, np.argwhere((got != want).any(-1) & ~aside)[:5].tolist())

    want, aside = ev.rank_counts(h, t, r, BAND)
    counts_agree("rank_triples", con.rank_triples(h, t, r)[0], want, aside)
    th, tt, tr = lp_order(g["test"])
    want, aside = ev.rank_counts(th, tt, tr, BAND)
    counts_agree("link_prediction", con.link_prediction()[0][:, :, :4], want, aside)
    want, aside = ev.relation_counts(th, tt, tr, BAND)
    counts_agree("relation_prediction", con.relation_prediction()[0], want, aside)

    p32 = {k: v.astype(np.float32) for k, v in case["params"].items()}
    ev32 = Evaluators(lambda a, b, c: scores(model, p32, a, b, c, De, Dr, "own_matrix", dtype=np.float32), g, case["lists"])
    worst = {"gpu": 0.0, "fp32": 0.0}

    def selection_agrees(name, ids, sc, want_ids, aside, rows64, rows32):
        shares[name] = max(shares.get(name, 0.0), float(aside.mean()))
        assert aside.mean() <= MAX_ASIDE, (name, aside.mean())
        for i in np.nonzero(~aside)[0]:
            assert set(ids[i].tolist()) == set(want_ids[i].tolist()), (name, i, ids[i].tolist(), want_ids[i].tolist())
            real = ids[i] >= 0
            assert np.isposinf(sc[i][~real]).all()
            s64 = rows64(i)[ids[i][real]]
            assert (np.abs(sc[i][real] - s64) <= RTOL * s64).all(), (name, i)
            worst["gpu"] = max(worst["gpu"], float((np.abs(sc[i][real] - s64) / s64).max()))
            worst["fp32"] = max(worst["fp32"], float((np.abs(rows32(i)[ids[i][real]].astype(np.float64) - s64) / s64).max()))

    for k in score_ref.RANDOM_K:
        for filtered in (False, True):
            for head, fixed, call in ((False, h, con.top_k_tails), (True, t, con.top_k_heads)):
                want_ids, _, aside = ev.top_k_entities(fixed, r, head, k, filtered, BAND)
                ids, sc = call(fixed, r, k, filtered=filtered)
                selection_agrees("top_k_entities", ids, sc, want_ids, aside, lambda i: ev.entity_scores(fixed[i], r[i], head)[0],
                                 lambda i: ev32.entity_scores(fixed[i], r[i], head)[0])
    for k in score_ref.RANDOM_K_REL:
        for filtered in (False, True):
            want_ids, _, aside = ev.top_k_relations(h, t, k, filtered, BAND)
            ids, sc = con.top_k_relations(h, t, k, filtered=filtered)
            selection_agrees("top_k_relations", ids, sc, want_ids, aside, lambda i: ev.relation_scores(h[i], t[i])[0],
                             lambda i: ev32.relation_scores(h[i], t[i])[0])
    parity_report("eval_definition[%s De=%d Dr=%d]" % (model, De, Dr), worst_gpu_rel_err=worst["gpu"], worst_fp32_numpy_rel_err=worst["fp32"],
                  ratio=worst["gpu"] / worst["fp32"] if worst["fp32"] else float("inf"), bound=RTOL, set_aside_share=shares, cap=MAX_ASIDE)


def tc_graph(model, params, E, R, De, Dr, seed):
    """Validation and test positives from the LOW score classes (the 80 lowest of 6000 random pairs per relation; the library
    draws the negatives as random typed tails, which land in the common, higher classes).  Relations 0..3 in both splits,
    relation 4 in the test split only (left out of the accuracy)."""
    rng = np.random.default_rng(seed)
    train = [rng.integers(0, E, 800), rng.integers(0, E, 800), rng.integers(0, R, 800)]
    valid, test = [], []
    for q in range(R):
        a, b = rng.integers(0, E, 6000), rng.integers(0, E, 6000)
        rr = np.full(6001, q); rr[0] = 0               # kge_predict's TransR matrix is the first triple's: relation 0 leads both lists
        s = exact_scores(model, params, np.concatenate([[0], a]), np.concatenate([[0], b]), rr, De, Dr, "predict")[1:]
        low = np.argsort(s, kind="stable")[:80]
        if q < 4:
            valid.append(np.stack([a[low[:40]], b[low[:40]], np.full(40, q)]))
        test.append(np.stack([a[low[40:]], b[low[40:]], np.full(40, q)]))
    valid, test = np.concatenate(valid, 1), np.concatenate(test, 1)
    return dict(E=E, R=R, train=tuple(train), valid=tuple(valid), test=tuple(test))


@pytest.mark.parametrize("model,De,Dr", [("transe", 64, 64), ("transh", 100, 100), ("transd", 200, 200), ("transr", 8, 260)])
def test_triple_classification_from_exact_scores(model, De, Dr):
    from tclass_cases import host_counts, numpy_fit
    E, R = score_ref.EVAL_E_EXACT, score_ref.EVAL_R
    params = score_ref.exact_tables(model, E, R, De, Dr)
    g = tc_graph(model, params, E, R, De, Dr, score_ref.seed_of("tc", model))
    con = engine_for(dict(graph=g, params=params), model, De, Dr, derive=True)
    res = con.triple_classification("test")
    batch = {k: getattr(con, k).copy() for k in ("valid_pos_h", "valid_pos_t", "valid_pos_r", "valid_neg_h", "valid_neg_t", "valid_neg_r",
                                                  "test_pos_h", "test_pos_t", "test_pos_r", "test_neg_h", "test_neg_t", "test_neg_r")}
    sc = {}
    for split in ("valid", "test"):
        for side in ("pos", "neg"):
            hh, tt, rr = (batch["%s_%s_%s" % (split, side, c)] for c in "htr")
            assert rr[0] == 0 and (np.diff(rr) >= 0).all()
            sc[split, side] = exact_scores(model, params, hh, tt, rr, De, Dr, "predict")
    assert np.median(sc["valid", "pos"]) < np.median(sc["valid", "neg"])         # two classes: the thresholds have something to find
    thresh = np.full(R, np.nan, np.float32)
    numpy_fit(batch["valid_pos_r"], sc["valid", "pos"], sc["valid", "neg"], thresh)
    tp, tn, fp, fn = host_counts(thresh, batch["valid_pos_r"], batch["test_pos_r"], sc["test", "pos"], sc["test", "neg"])
    assert (res["tp"], res["tn"], res["fp"], res["fn"]) == (tp, tn, fp, fn)
    assert tp + fn == 160 and tp + tn > fp + fn                                   # relation 4 is left out; better than chance
    assert res["acc"] == float(np.float32((tp + tn) / (tp + tn + fp + fn)))
    assert np.array_equal(con.relThresh[:4].view(np.uint32), thresh[:4].view(np.uint32)), (con.relThresh, thresh)
