"""TransR on relation-grouped shared negatives, the host side: which plan step_plan gives it once the library says the entry point
takes the shape (kge_shared_transr_supported, the keyword shared_transr_supported), every configuration that stays refused with
the limit it names, and the library's answer itself.  No GPU."""
import pytest

from openkeonspark_amd import KgeError, step_plan
from openkeonspark_amd._lib import TRANSD, TRANSE, TRANSH, TRANSR

BASE = dict(model_id=TRANSR, opt_method="SGD", sparse_rows=None, use_counts=True, counts_supported=0, ent_total=993, rel_total=7,
            width=64, batch_size=128, n_neg=25, shared_chunk=64, negative_rel=0, by_relation=True)


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("opt,kind", [("SGD", "sgd"), ("Adagrad", "adagrad"), ("Adam", "adam")])
def test_the_plan_is_transrs_dense_plan(opt, kind, typed):
    p = step_plan.plan(**dict(BASE, opt_method=opt, typed=typed, shared_transr_supported=1))
    assert p.optimizer == kind and not p.sparse_inplace and not p.sparse_rows and not p.use_counts
    # ... the plan its unshared step has, whatever the caller wished for the sign-count path
    unshared = dict(BASE, opt_method=opt, shared_chunk=0, by_relation=False)
    assert p == step_plan.plan(**unshared) == step_plan.StepPlan(kind, False, False, False, p.table_bytes)
    for wish in (dict(use_counts=False), dict(sparse_rows=False)):
        assert step_plan.plan(**dict(BASE, opt_method=opt, typed=typed, shared_transr_supported=1, **wish)) == p


def test_lazy_adam_stays_refused_in_its_existing_words():
    with pytest.raises(KgeError) as shared:
        step_plan.plan(**dict(BASE, opt_method="LazyAdam", shared_transr_supported=1))
    with pytest.raises(KgeError) as unshared:
        step_plan.plan(**dict(BASE, opt_method="LazyAdam", shared_chunk=0, by_relation=False))
    assert str(shared.value) == str(unshared.value) and "LazyAdam" in str(shared.value) and "no record path" in str(shared.value)


def test_without_the_librarys_answer_every_refusal_keeps_its_words():
    for kw in ({}, dict(shared_transr_supported=0), dict(shared_float_supported=1), dict(shared_transd_supported=1),
               dict(shared_float_supported=1, shared_transd_supported=1, shared_transr_supported=0)):
        with pytest.raises(KgeError, match="TransE only: TransH, TransD and TransR have no shared emit kernel"):
            step_plan.plan(**dict(BASE, **kw))
    with pytest.raises(KgeError, match="TransE only"):
        step_plan.check_shared_negatives(TRANSR, "sgd", True, 64, 25, 0, True, False)
    with pytest.raises(KgeError, match="TransE only"):
        step_plan.check_shared_negatives(TRANSR, "sgd", True, 64, 25, 0, True, False, 1, 1)      # the other two answers open nothing
    step_plan.check_shared_negatives(TRANSR, "sgd", False, 64, 25, 0, True, False, 0, 0, 1)      # taken, and needs no use_counts
    step_plan.check_shared_negatives(TRANSR, "adam", False, 64, 25, 0, True, True, 0, 0, 1)      # ... with TF1 Adam and typed, too


def test_the_answer_for_transr_opens_no_other_model():
    te = dict(BASE, model_id=TRANSE, counts_supported=1)
    assert step_plan.plan(**te) == step_plan.plan(**dict(te, shared_transr_supported=1)) == step_plan.StepPlan("sgd", True, True, False, 256000)
    with pytest.raises(KgeError, match="SGD, LazyAdam or Adagrad"):      # TransE keeps its refusal of TF1 Adam
        step_plan.plan(**dict(te, opt_method="Adam", shared_transr_supported=1))
    for model_id in (TRANSH, TRANSD):
        with pytest.raises(KgeError, match="TransE only"):
            step_plan.plan(**dict(BASE, model_id=model_id, shared_transr_supported=1))
    # the other models' answers keep working beside it
    assert step_plan.plan(**dict(BASE, model_id=TRANSH, shared_float_supported=1, shared_transr_supported=1)).sparse_inplace
    assert step_plan.plan(**dict(BASE, model_id=TRANSD, shared_transd_supported=1, shared_transr_supported=1)).sparse_inplace


@pytest.mark.parametrize("supported", [0, 1])
def test_chunks_by_position_stay_refused(supported):
    with pytest.raises(KgeError, match="TransE only") as exc:
        step_plan.plan(**dict(BASE, by_relation=False, shared_transr_supported=supported))
    if supported:      # in the words of TransH's and TransD's refusal: the way out is named
        assert "by_relation=True" in str(exc.value) and "TransR shares one matrix per chunk" in str(exc.value) and "chunks by position" in str(exc.value)


@pytest.mark.parametrize("change,word", [
    (dict(negative_rel=1, n_neg=26), "negative_rel"),
    (dict(n_neg=64), "1 to 63"),
    (dict(shared_chunk=128), "1 to 127"),
    (dict(n_neg=0), "1 to 63"),
    (dict(typed=True, by_relation=False), "type-constrained"),
])
def test_refusals_name_their_limit(change, word):
    with pytest.raises(KgeError, match="shared negatives") as exc:
        step_plan.plan(**dict(BASE, shared_transr_supported=1, **change))
    assert word in str(exc.value)


def test_the_library_answers_for_transr_alone():
    """kge_shared_transr_supported: TransR, negative_rel == 0, 1 <= N <= 63, rel_dim <= 512, any ent_dim (a host function).  The
    symbol is this feature's: the test fails where the library lacks it."""
    import ctypes
    from openkeonspark_amd import _lib
    L = _lib.lib()

    def desc(**kw):
        d = _lib.ModelDesc()
        d.model = TRANSR; d.negative_rel = 0; d.ent_total = 100; d.rel_total = 7; d.ent_dim = 200; d.rel_dim = 200; d.margin = 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def ask(N=25, **kw):
        return L.kge_shared_transr_supported(ctypes.byref(desc(**kw)), N)

    assert ask() == 1 and ask(1) == 1 and ask(63) == 1 and ask(rel_dim=512) == 1 and ask(ent_dim=50, rel_dim=18) == 1 and ask(ent_dim=1000) == 1
    assert ask(0) == 0 and ask(64) == 0 and ask(negative_rel=1) == 0 and ask(rel_dim=516) == 0 and ask(rel_dim=0) == 0 and ask(ent_dim=0) == 0
    for model in (TRANSE, TRANSH, TRANSD):
        assert ask(model=model) == 0
    assert L.kge_shared_transr_supported(None, 25) == 0
    # the three answers do not overlap
    assert L.kge_shared_float_supported(ctypes.byref(desc()), 25) == 0 and L.kge_shared_transd_supported(ctypes.byref(desc()), 25) == 0
