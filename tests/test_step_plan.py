"""step_plan: the path a training step takes, from plain values.  The expected plans below are literals, written from the rules
(and checked on the device against Config's flags in test_gpu_step_plan.py); nothing here needs a GPU or the engine library."""
import itertools

import pytest

from openkeonspark_amd import KgeError, step_plan

TRANSE, TRANSH, TRANSR, TRANSD = 0, 1, 2, 3
VECTOR = {"TransE": TRANSE, "TransH": TRANSH, "TransD": TRANSD}
SPELLINGS = {"sgd": ["SGD", "sgd", "RMSProp"],      # (no name is "SGD": every name that is no other optimizer's trains with it)
             "adam": ["Adam", "adam"],
             "lazy_adam": ["LazyAdam", "lazyadam", "lazy_adam"],
             "adagrad": ["Adagrad", "adagrad"]}
WISHES = (None, True, False)

LAZY_ERR = ("LazyAdam (touched rows only, NON-PARITY) needs TransE, TransH or TransD: TransR's gradient is a whole "
            "matrix per relation and has no record path")
SPARSE_ERR = "sparse_rows needs TransE / TransH / TransD with SGD, LazyAdam or Adagrad"

# An outcome is three letters, (use_counts, sparse_rows, sparse_inplace) as "c" / "r" / "i" or "-", or the text of the KgeError.
# A small table (E + R = 1000 rows of 64 floats, batch 128, one negative: below every size rule), `use_counts` wished for:
#   kind, counts_supported, TransE / TransH / TransD with sparse_rows None, True, False, TransR with sparse_rows None, True, False
SMALL = [
    ("sgd",       0, ("---", "--i", "---"),            ("---", SPARSE_ERR, "---")),
    ("sgd",       1, ("c--", "cr-", "c--"),            ("c--", "cr-", "c--")),
    ("adam",      0, ("---", SPARSE_ERR, "---"),       ("---", SPARSE_ERR, "---")),
    ("adam",      1, ("c--", SPARSE_ERR, "c--"),       ("c--", SPARSE_ERR, "c--")),
    ("lazy_adam", 0, ("--i", "--i", "--i"),            (LAZY_ERR, LAZY_ERR, LAZY_ERR)),
    ("lazy_adam", 1, ("cr-", "cr-", "cr-"),            ("cr-", "cr-", "cr-")),
    ("adagrad",   0, ("--i", "--i", "--i"),            ("---", SPARSE_ERR, "---")),
    ("adagrad",   1, ("cr-", "cr-", "cr-"),            ("cr-", "cr-", "cr-")),
]

ROW = 64 * 4                     # bytes of a row at width 64
FLOOR_ROWS = (128 << 20) // ROW          # 524 288 rows = 128 MB exactly
TOUCHED_ROWS = 1258291           # batch 2^20, one negative: 0.3 * (2^20 * 4 rows) * 256 B = 322 122 547.2 B = 1 258 291.2 rows
INPLACE_ROWS = (2 << 30) // ROW          # 8 388 608 rows = 2 GB exactly
# sparse_rows left at None, `use_counts` wished for: just below (at) and just above each size in the rule
#   model, optimizer, counts_supported, rows E + R, batch, sparse_threshold_bytes, outcome
SIZES = [
    ("TransE", "SGD",     1, FLOOR_ROWS,       128,     None,       "c--"),      # the 128 MB floor
    ("TransE", "SGD",     1, FLOOR_ROWS + 1,   128,     None,       "cr-"),
    ("TransE", "Adagrad", 1, FLOOR_ROWS,       128,     None,       "cr-"),      # (a rows rule does not wait for a size)
    ("TransE", "Adam",    1, FLOOR_ROWS + 1,   128,     None,       "c--"),      # (Adam sweeps every row: never sparse)
    ("TransE", "SGD",     1, TOUCHED_ROWS,     1 << 20, None,       "c--"),      # 0.3 x the bytes of the rows a step touches
    ("TransE", "SGD",     1, TOUCHED_ROWS + 1, 1 << 20, None,       "cr-"),
    ("TransE", "SGD",     1, 1000,             128,     1000 * ROW, "c--"),      # an explicit sparse_threshold_bytes
    ("TransE", "SGD",     1, 1001,             128,     1000 * ROW, "cr-"),
    ("TransE", "SGD",     1, 1001,             1 << 20, 1000 * ROW, "cr-"),      # (... replaces both measured rules)
    ("TransE", "SGD",     1, FLOOR_ROWS + 1,   128,     1 << 40,    "c--"),
    ("TransH", "SGD",     0, FLOOR_ROWS + 1,   128,     None,       "---"),      # no sign counts: no sparse rows; in place from 2 GB
    ("TransH", "SGD",     0, INPLACE_ROWS,     128,     None,       "---"),
    ("TransH", "SGD",     0, INPLACE_ROWS + 1, 128,     None,       "--i"),
    ("TransD", "sgd",     0, INPLACE_ROWS + 1, 128,     None,       "--i"),
    ("TransE", "SGD",     0, INPLACE_ROWS + 1, 128,     None,       "--i"),
    ("TransR", "SGD",     0, INPLACE_ROWS + 1, 128,     None,       "---"),
    ("TransH", "Adam",    0, INPLACE_ROWS + 1, 128,     None,       "---"),
    ("TransE", "SGD",     1, INPLACE_ROWS + 1, 128,     None,       "cr-"),      # (sparse rows come first)
    ("TransE", "SGD",     1, INPLACE_ROWS,     128,     1 << 40,    "c--"),      # sign counts, kept off sparse rows by the threshold
    ("TransE", "SGD",     1, INPLACE_ROWS + 1, 128,     1 << 40,    "c-i"),
]


def outcome(**kw):
    args = dict(model_id=TRANSE, opt_method="SGD", sparse_rows=None, use_counts=True, counts_supported=1, ent_total=993, rel_total=7,
                width=64, batch_size=128, n_neg=1)
    args.update(kw)
    try:
        p = step_plan.plan(**args)
    except KgeError as exc:
        return str(exc), None
    return ("c" if p.use_counts else "-") + ("r" if p.sparse_rows else "-") + ("i" if p.sparse_inplace else "-"), p


def test_small_table_grid():
    seen = 0
    for kind, supported, vector, transr in SMALL:
        models = [(name, mid, vector) for name, mid in VECTOR.items()] + [("TransR", TRANSR, transr)]
        for (name, mid, want), spelling, wish in itertools.product(models, SPELLINGS[kind], range(3)):
            got, p = outcome(model_id=mid, opt_method=spelling, sparse_rows=WISHES[wish], counts_supported=supported)
            assert got == want[wish], (name, spelling, WISHES[wish], supported)
            seen += 1
            if p is not None:
                assert p.optimizer == kind and p.table_bytes == 1000 * ROW
                assert (p.adam, p.lazy_adam, p.adagrad) == (kind == "adam", kind == "lazy_adam", kind == "adagrad")
                assert p.has_slots == (kind in ("adam", "lazy_adam")) and p.rows_rule == (kind in ("lazy_adam", "adagrad"))
                # `use_counts` not wished for: no sign counts, and with them no sparse rows -- the in-place rows take over
                off, _ = outcome(model_id=mid, opt_method=spelling, sparse_rows=WISHES[wish], counts_supported=supported, use_counts=False)
                on0, _ = outcome(model_id=mid, opt_method=spelling, sparse_rows=WISHES[wish], counts_supported=0)
                assert off == on0, (name, spelling, WISHES[wish], supported)
    assert seen == 4 * 10 * 3 * 2


@pytest.mark.parametrize("model,opt,supported,rows,batch,threshold,expected", SIZES)
def test_size_thresholds(model, opt, supported, rows, batch, threshold, expected):
    mid = dict(VECTOR, TransR=TRANSR)[model]
    got, p = outcome(model_id=mid, opt_method=opt, counts_supported=supported, ent_total=rows - 7, rel_total=7, batch_size=batch,
                     sparse_threshold_bytes=threshold)
    assert got == expected
    assert p.table_bytes == rows * ROW
    assert isinstance(p, tuple) and not hasattr(p, "__dict__")      # immutable
    with pytest.raises(AttributeError):
        p.sparse_rows = True


def test_optimizer_names():
    for kind, names in SPELLINGS.items():
        for name in names:
            assert step_plan.optimizer_kind(name) == kind
    for name in ("ADAM", "Lazy_Adam", "AdaGrad", "", None):      # (no other spelling is accepted: SGD)
        assert step_plan.optimizer_kind(name) == "sgd"


@pytest.mark.parametrize("kw,text", [
    (dict(model_id=TRANSR, opt_method="LazyAdam", counts_supported=0), LAZY_ERR),
    (dict(model_id=TRANSR, opt_method="SGD", counts_supported=0, sparse_rows=True), SPARSE_ERR),
    (dict(opt_method="Adagrad", adagrad_initial_accumulator=0.0),
     "adagrad_initial_accumulator must be positive (the Adagrad rule divides by sqrt(accumulator), without an epsilon), got 0.0"),
    (dict(opt_method="adagrad", adagrad_initial_accumulator=-1),
     "adagrad_initial_accumulator must be positive (the Adagrad rule divides by sqrt(accumulator), without an epsilon), got -1"),
])
def test_errors(kw, text):
    with pytest.raises(KgeError) as err:
        step_plan.plan(**dict(dict(model_id=TRANSE, sparse_rows=None, use_counts=True, counts_supported=1, ent_total=993, rel_total=7,
                                   width=64, batch_size=128, n_neg=1), **kw))
    assert str(err.value) == text
    # (an accumulator that is not positive matters to Adagrad alone)
    assert outcome(opt_method="SGD", adagrad_initial_accumulator=0.0)[0] == "c--"


def test_shards_at_creation():
    rows = outcome(sparse_rows=True)[1]                               # "cr-": the step that shards its table
    dense = outcome()[1]                                              # "c--"
    inplace = outcome(counts_supported=0, sparse_rows=True)[1]        # "--i"
    #   world, width, sharded?
    for world, width, want in [(1, 8, False), (2, 8, True), (64, 8, True), (65, 8, False),
                               (1, 6, False), (2, 6, False), (64, 6, False), (65, 6, False)]:
        assert step_plan.shards_at_creation(rows, TRANSE, world, width) is want, (world, width)
        assert step_plan.shards_at_creation(dense, TRANSE, world, width) is False
        assert step_plan.shards_at_creation(inplace, TRANSE, world, width) is False
        assert step_plan.shards_at_creation(rows, TRANSH, world, width) is False


def test_large_counts_step_boundary():
    counts, rows = outcome()[1], outcome(sparse_rows=True)[1]
    inplace_counts = outcome(ent_total=INPLACE_ROWS - 6, sparse_threshold_bytes=1 << 40)[1]      # "c-i"
    atomics = outcome(counts_supported=0)[1]
    # 100 positives with 2 negatives each: 500 gradient rows; counts_min_records 250 on 2 ranks: 500
    assert step_plan.large_counts_step(counts, 100, 2, 250, 2) is True
    assert step_plan.large_counts_step(counts, 99, 2, 250, 2) is False           # 495
    assert step_plan.large_counts_step(counts, 100, 2, 251, 2) is False
    assert step_plan.large_counts_step(counts, 100, 2, 500, 1) is True
    assert step_plan.large_counts_step(counts, 1, 0, 0, 8) is True               # counts_min_records = 0: always
    for other in (rows, inplace_counts, atomics):                                # only the dense sign-count step has the predicate
        assert step_plan.large_counts_step(other, 100, 2, 0, 1) is False
