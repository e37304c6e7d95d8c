"""step_plan with shared negatives (Config.set_shared_negatives): every refusal names its limit, accepted shapes take the
sparse-rows record step whatever the table size, and with the option off plan() returns what it returned before, for every case
tests/test_step_plan.py lists.  No GPU."""
import itertools

import pytest

from openkeonspark_amd import KgeError, step_plan
from test_step_plan import SIZES, SMALL, SPELLINGS, TRANSD, TRANSE, TRANSH, TRANSR, VECTOR, WISHES, outcome

BASE = dict(model_id=TRANSE, opt_method="SGD", sparse_rows=None, use_counts=True, counts_supported=1, ent_total=993, rel_total=7,
            width=64, batch_size=128, n_neg=25, shared_chunk=64, negative_rel=0)


def plan(**kw):
    return step_plan.plan(**dict(BASE, **kw))


@pytest.mark.parametrize("change,words", [
    (dict(opt_method="Adam"), ["TF1 Adam", "the dense count image has no entrance for shared records yet"]),
    (dict(model_id=TRANSH, counts_supported=0), ["TransE only", "TransH"]),
    (dict(model_id=TRANSD, counts_supported=0), ["TransE only", "TransD"]),
    (dict(model_id=TRANSR, counts_supported=0), ["TransE only", "TransR"]),
    (dict(n_neg=26, negative_rel=1), ["relation negatives", "negative_rel must be 0"]),
    (dict(n_neg=64, counts_supported=0), ["63", "got 64"]),
    (dict(shared_chunk=128), ["127", "got 128"]),
    (dict(shared_chunk=-1), ["127"]),
    (dict(use_counts=False), ["sign-count"]),
    (dict(counts_supported=0), ["sign-count"]),
])
def test_refusals_name_the_limit(change, words):
    with pytest.raises(KgeError) as exc:
        plan(**change)
    for w in words:
        assert w in str(exc.value), (w, str(exc.value))


@pytest.mark.parametrize("opt", ["SGD", "LazyAdam", "Adagrad"])
@pytest.mark.parametrize("wish", WISHES)
@pytest.mark.parametrize("chunk,n_neg", [(1, 1), (64, 25), (127, 63)])
@pytest.mark.parametrize("rows", [1000, 50_000_000])
def test_accepted_shapes_take_the_sparse_rows_step(opt, wish, chunk, n_neg, rows):
    p = plan(opt_method=opt, sparse_rows=wish, shared_chunk=chunk, n_neg=n_neg, ent_total=rows - 7)
    assert p.use_counts and p.sparse_rows and not p.sparse_inplace
    assert p.optimizer == step_plan.optimizer_kind(opt) and p.table_bytes == rows * 64 * 4


def test_off_is_the_plan_as_it_was():
    """shared_chunk = 0 (and the argument left out) against the literals of tests/test_step_plan.py, and against each other."""
    seen = 0
    for kind, supported, vector, transr in SMALL:
        models = [(mid, vector) for mid in VECTOR.values()] + [(TRANSR, transr)]
        for (mid, want), spelling, wish in itertools.product(models, SPELLINGS[kind], range(3)):
            kw = dict(model_id=mid, opt_method=spelling, sparse_rows=WISHES[wish], counts_supported=supported)
            got, p = outcome(shared_chunk=0, negative_rel=0, **kw)
            assert got == want[wish]
            assert p == outcome(**kw)[1]
            seen += 1
    for model, opt, supported, rows, batch, threshold, expected in SIZES:
        kw = dict(model_id=dict(VECTOR, TransR=TRANSR)[model], opt_method=opt, counts_supported=supported, ent_total=rows - 7,
                  rel_total=7, batch_size=batch, sparse_threshold_bytes=threshold)
        got, p = outcome(shared_chunk=0, **kw)
        assert got == expected and p == outcome(**kw)[1]
        seen += 1
    assert seen == 4 * 10 * 3 * 2 + len(SIZES)


def test_config_refusals_before_a_model():
    """What Config refuses without a device: a chunk outside 1..127, typed sampling in either order."""
    import openkeonspark_amd as ok
    con = ok.Config()
    with pytest.raises(KgeError, match="127"):
        con.set_shared_negatives(128)
    con.set_shared_negatives(64, seed=5)
    assert (con._shared_chunk, con._shared_seed) == (64, 5)
    with pytest.raises(KgeError, match="type-constrained"):
        con.set_type_constrained_sampling(True)
    con.set_shared_negatives(0)
    assert con._shared_chunk == 0
    con.set_type_constrained_sampling(True)
    with pytest.raises(KgeError, match="type-constrained"):
        con.set_shared_negatives(16)
