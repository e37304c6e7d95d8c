"""bf16 table storage together with shared negatives, without a device: what step_plan.plan makes of the two wishes, every
refusal with its reason, the driver's switches and the two checkpoint records side by side."""
import numpy as np
import pytest

from openkeonspark_amd import step_plan
from openkeonspark_amd._lib import KgeError, TRANSE, TRANSH, TRANSD, TRANSR

E, R, D = 500, 7, 24
BASE = dict(model_id=TRANSE, opt_method="SGD", sparse_rows=None, use_counts=True, counts_supported=1, ent_total=E, rel_total=R,
            width=D, batch_size=301, n_neg=5, table_dtype="bf16", bf16_supported=1, shared_chunk=16, bf16_shared_supported=1)


@pytest.mark.parametrize("grouped", [dict(), dict(by_relation=True), dict(by_relation=True, typed=True),
                                     dict(by_relation=True, in_chunk=2), dict(by_relation=True, typed=True, in_chunk=2)])
@pytest.mark.parametrize("opt,kind", [("SGD", "sgd"), ("RowAdagrad", "row_adagrad")])
def test_the_two_wishes_give_the_sparse_rows_record_plan(opt, kind, grouped):
    """TransE with SGD or RowAdagrad, chunks by position or by relation: the int8-record touched-rows plan, 2 (E + R) D table bytes."""
    p = step_plan.plan(**dict(BASE, opt_method=opt, **grouped))
    assert p == step_plan.StepPlan(kind, True, True, False, 2 * (E + R) * D)
    for wish in (True, False):      # (like either mode alone: whatever `sparse_rows` says)
        assert p == step_plan.plan(**dict(BASE, opt_method=opt, sparse_rows=wish, **grouped))


def test_either_mode_off_plans_as_before():
    """The new answer is read only where both modes are on."""
    for answer in (0, 1):
        kw = dict(BASE, bf16_shared_supported=answer)
        assert step_plan.plan(**dict(kw, shared_chunk=0)) == step_plan.StepPlan("sgd", True, True, False, 2 * (E + R) * D)
        assert step_plan.plan(**dict(kw, table_dtype="fp32")) == step_plan.StepPlan("sgd", True, True, False, 4 * (E + R) * D)
        assert step_plan.plan(**dict(kw, table_dtype="fp32", opt_method="LazyAdam")).optimizer == "lazy_adam"


@pytest.mark.parametrize("change,reason", [
    (dict(bf16_shared_supported=0), "kge_bf16_shared_supported refuses"),
    (dict(width=520), "up to 512"),
    (dict(width=1024), "up to 512"),
    (dict(negative_rel=1), "negative_rel must be 0"),
    (dict(opt_method="LazyAdam"), "needs SGD or RowAdagrad"),
    (dict(opt_method="Adagrad"), "needs SGD or RowAdagrad"),
    (dict(opt_method="Adam"), "needs SGD or RowAdagrad"),
    (dict(model_id=TRANSH, counts_supported=0, by_relation=True, shared_float_supported=1), "their tables stay fp32"),
    (dict(model_id=TRANSD, counts_supported=0, by_relation=True, shared_transd_supported=1), "their tables stay fp32"),
    (dict(model_id=TRANSR, counts_supported=0, by_relation=True, shared_transr_supported=1), "their tables stay fp32"),
    (dict(width=100), "multiple of 8"),
    (dict(use_counts=False), "sign-count path"),
])
def test_refusals_name_the_limit(change, reason):
    with pytest.raises(KgeError) as e:
        step_plan.plan(**dict(BASE, **change))
    assert reason in str(e.value) and "bf16" in str(e.value)


@pytest.mark.parametrize("change,reason", [
    (dict(shared_chunk=128), "1 to 127 positives"),
    (dict(n_neg=64), "1 to 63 negatives"),
    (dict(by_relation=True, in_chunk=59), "at most 63"),
    (dict(in_chunk=2), "in-chunk candidates need chunks of one relation"),
    (dict(typed=True), "type-constrained sampling"),
])
def test_the_shared_steps_own_limits_still_hold(change, reason):
    with pytest.raises(KgeError) as e:
        step_plan.plan(**dict(BASE, **change))
    assert reason in str(e.value)


def test_equal_seeds_are_refused():
    """Both hashes start from mix(seed + (step + 1) G): one seed for both would round rows with the bits that drew candidates."""
    step_plan.check_bf16_shared_seeds(1, 2)
    step_plan.check_bf16_shared_seeds(0, 2 ** 63)
    for seed in (0, 7, 2 ** 64 - 1):
        with pytest.raises(KgeError) as e:
            step_plan.check_bf16_shared_seeds(seed, seed)
        assert "shared negatives" in str(e.value) and "bf16" in str(e.value) and "must differ" in str(e.value)
    import bf16_ref
    import shared_neg_ref
    assert int(bf16_ref.step_key(7, 3)) == shared_neg_ref.step_key(7, 3) and int(bf16_ref.step_key(7, 3)) != shared_neg_ref.step_key(8, 3)


def test_more_than_one_rank_is_refused():
    """The plan knows no world size: Config refuses it, before and after the model is made (a setter and a stub suffice)."""
    import openkeonspark_amd as pkg
    con = pkg.Config.__new__(pkg.Config)
    con.set_table_dtype("bf16", seed=9)
    con.world_size = 2
    with pytest.raises(KgeError) as e:
        con._refuse_bf16_ranks()
    assert "single-process only" in str(e.value) and "bf16" in str(e.value)


def test_the_driver_takes_the_two_switches_together():
    from openkeonspark_amd import distribute_training as dt
    for argv in (["--table_dtype", "bf16", "--shared_negatives_chunk", "16"], ["--shared_negatives_chunk", "16", "--table_dtype", "bf16"]):
        a = dt.parse_args(argv + ["--table_rounding_seed", "77", "--shared_negatives_seed", "5", "--shared_negatives_by_relation", "1",
                                  "--shared_negatives_in_chunk", "2"])
        assert (a.table_dtype, a.table_rounding_seed, a.shared_negatives_chunk, a.shared_negatives_seed) == ("bf16", 77, 16, 5)
        assert a.shared_negatives_by_relation == 1 and a.shared_negatives_in_chunk == 2


def test_setters_in_either_order():
    import openkeonspark_amd as pkg
    for order in (0, 1):
        con = pkg.Config.__new__(pkg.Config)
        con.trainModel, con.type_constrained_sampling = None, False
        calls = [lambda: con.set_table_dtype("bf16", seed=3), lambda: con.set_shared_negatives(16, seed=4, by_relation=True, in_chunk=2)]
        for call in calls[::-1] if order else calls:
            call()
        assert con._bf16 and (con._table_seed, con._shared_chunk, con._shared_seed, con._shared_by_relation, con._shared_in_chunk) == (3, 16, 4, True, 2)


class _Run(object):
    type_constrained_sampling = False

    def __init__(self, bf16, table_seed, chunk, seed, by_relation=False, in_chunk=0):
        self._bf16, self._table_seed = bf16, table_seed
        self._shared_chunk, self._shared_seed, self._shared_by_relation, self._shared_in_chunk = chunk, seed, by_relation, in_chunk


def test_both_checkpoint_records_are_checked_on_resume():
    from openkeonspark_amd import distribute_training as dt
    run = _Run(True, 11, 16, 5)
    z = {"table_dtype": dt.table_dtype_record(run), "shared_negatives": dt.shared_negatives_record(run)}
    assert [int(x) for x in z["table_dtype"]] == [1, 11] and [int(x) for x in z["shared_negatives"]][:2] == [16, 5]

    def check(con):
        dt.check_shared_negatives_record(z, con)
        dt.check_table_dtype_record(z, con)

    check(_Run(True, 11, 16, 5))
    for other, words in ((_Run(True, 12, 16, 5), "rounding seed"), (_Run(True, 11, 8, 5), "shared negatives"),
                         (_Run(True, 11, 16, 6), "shared negatives"), (_Run(True, 11, 0, 0), "shared negatives")):
        with pytest.raises(KgeError) as e:
            check(other)
        assert words in str(e.value)
    grouped = _Run(True, 11, 16, 5, by_relation=True, in_chunk=2)
    z = {"table_dtype": dt.table_dtype_record(grouped), "shared_negatives": dt.shared_negatives_record(grouped)}
    check(grouped)
    with pytest.raises(KgeError):
        check(_Run(True, 11, 16, 5, by_relation=True, in_chunk=3))
    assert isinstance(z["shared_negatives"], np.ndarray)
