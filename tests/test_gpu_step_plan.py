"""Config.set_model_and_session sets its path flags from step_plan.plan: for one configuration per distinct plan outcome, the
flags of a real Config equal the pure function's plan for the same inputs (tests/test_step_plan.py pins the plans themselves)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, R, D, BATCH = 60, 5, 8, 32
TABLE_BYTES = (E + R) * D * 4

#   model, optimizer, attributes set before the session -> (use_counts, sparse_rows, sparse_inplace) as "c" / "r" / "i", or the error
CASES = [
    ("TransE", "SGD",      {},                                                  "c--"),
    ("TransE", "Adam",     {},                                                  "c--"),
    ("TransE", "SGD",      dict(sparse_threshold_bytes=TABLE_BYTES),            "c--"),      # at the threshold
    ("TransE", "SGD",      dict(sparse_threshold_bytes=TABLE_BYTES - 1),        "cr-"),      # above it
    ("TransE", "sgd",      dict(sparse_rows=True),                              "cr-"),
    ("TransE", "Adam",     dict(sparse_threshold_bytes=0),                      "c--"),
    ("TransE", "LazyAdam", dict(sparse_rows=False),                             "cr-"),
    ("TransE", "adagrad",  {},                                                  "cr-"),
    ("TransE", "SGD",      dict(use_counts=False),                              "---"),
    ("TransE", "SGD",      dict(use_counts=False, sparse_rows=True),            "--i"),
    ("TransE", "SGD",      dict(use_counts=False, sparse_threshold_bytes=0),    "---"),      # (sparse rows wanted, but no sign counts)
    ("TransH", "SGD",      {},                                                  "---"),
    ("TransH", "adam",     {},                                                  "---"),
    ("TransH", "SGD",      dict(sparse_rows=True),                              "--i"),
    ("TransD", "lazyadam", {},                                                  "--i"),
    ("TransH", "Adagrad",  {},                                                  "--i"),
    ("TransR", "SGD",      {},                                                  "---"),
    ("TransR", "Adagrad",  {},                                                  "---"),
    ("TransR", "RMSProp",  {},                                                  "---"),
    ("TransR", "LazyAdam", {},                                                  "LazyAdam (touched rows only"),
    ("TransR", "SGD",      dict(sparse_rows=True),                              "sparse_rows needs TransE"),
    ("TransH", "Adam",     dict(sparse_rows=True),                              "sparse_rows needs TransE"),
    ("TransH", "Adagrad",  dict(adagrad_initial_accumulator=0.0),               "adagrad_initial_accumulator must be positive"),
]


@pytest.fixture(scope="module")
def triples():
    """4 * BATCH distinct (h, t, r)."""
    rng = np.random.default_rng(60)
    ids = rng.choice(E * E * R, 4 * BATCH, replace=False)
    return ids // (E * R), ids // R % E, ids % R


@pytest.mark.parametrize("model,opt,attrs,expected", CASES)
def test_config_flags_are_the_plan(triples, model, opt, attrs, expected):
    import openkeonspark_amd as pkg
    from openkeonspark_amd import step_plan
    con = pkg.Config()
    con.set_work_threads(4); con.set_dimension(D); con.set_nbatches(4); con.set_ent_neg_rate(1); con.set_opt_method(opt)
    for k, v in attrs.items():
        setattr(con, k, v)
    con.init_from_arrays(E, R, *triples)
    cls = getattr(pkg, model)
    desc = cls(config=con, define=False).descriptor()
    args = (cls.model_id, opt, attrs.get("sparse_rows"), attrs.get("use_counts", True),
            con.lib.kge_transe_counts_supported(ctypes.byref(desc), 1), E, R, D, con.batch_size, 1, attrs.get("sparse_threshold_bytes"),
            attrs.get("adagrad_initial_accumulator", 0.1))
    if len(expected) > 3:
        with pytest.raises(pkg.KgeError) as from_plan:
            step_plan.plan(*args)
        with pytest.raises(pkg.KgeError) as from_config:
            con.set_model_and_session(cls)
        assert str(from_plan.value) == str(from_config.value) and str(from_plan.value).startswith(expected)
        return
    p = step_plan.plan(*args)
    con.set_model_and_session(cls)
    assert con.batch_size == BATCH and p.table_bytes == TABLE_BYTES
    assert ("c" if p.use_counts else "-") + ("r" if p.sparse_rows else "-") + ("i" if p.sparse_inplace else "-") == expected
    assert (con.use_counts, con.sparse_rows, con.sparse_inplace) == (p.use_counts, p.sparse_rows, p.sparse_inplace)
    assert (con._adam, con._lazy_adam, con._adagrad, con._has_slots) == (p.adam, p.lazy_adam, p.adagrad, p.has_slots)
    assert (con._grads == []) == (p.sparse_rows or p.sparse_inplace)
    for flag in (con.use_counts, con.sparse_rows, con.sparse_inplace, con._adam, con._lazy_adam, con._adagrad, con._has_slots):
        assert type(flag) is bool
