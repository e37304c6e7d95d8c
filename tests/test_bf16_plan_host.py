"""bf16 table storage without a device: what step_plan.plan makes of the wish, every refusal with its reason, and the numpy
restatement of the stochastic rounding rule (tests/bf16_ref.py) against the properties the definition states."""
import numpy as np
import pytest

import bf16_ref as ref
from openkeonspark_amd import step_plan
from openkeonspark_amd._lib import KgeError, TRANSE, TRANSH, TRANSD, TRANSR

BASE = dict(model_id=TRANSE, opt_method="SGD", sparse_rows=None, use_counts=True, counts_supported=1, ent_total=500, rel_total=7,
            width=24, batch_size=301, n_neg=5, table_dtype="bf16", bf16_supported=1)


@pytest.mark.parametrize("opt,kind", [("SGD", "sgd"), ("RowAdagrad", "row_adagrad")])
@pytest.mark.parametrize("wish", [None, True, False])
def test_the_wish_gives_the_sparse_rows_plan(opt, kind, wish):
    """TransE with SGD or RowAdagrad: the int8-record touched-rows plan whatever the table size and `sparse_rows` say (a table
    of 24 KB would be dense without the wish), with the table's bytes halved."""
    p = step_plan.plan(**dict(BASE, opt_method=opt, sparse_rows=wish))
    assert p == step_plan.StepPlan(kind, True, True, False, (500 + 7) * 24 * 2)
    off = step_plan.plan(**dict(BASE, opt_method=opt, sparse_rows=wish, table_dtype="fp32"))
    assert off.table_bytes == (500 + 7) * 24 * 4 and off == step_plan.plan(**dict(BASE, opt_method=opt, sparse_rows=wish, table_dtype="fp32",
                                                                                 bf16_supported=0))
    if wish is None and opt == "SGD":
        assert not off.sparse_rows


def test_the_default_is_fp32_and_changes_no_plan():
    kw = {k: v for k, v in BASE.items() if k not in ("table_dtype", "bf16_supported")}
    for opt in ("SGD", "Adam", "LazyAdam", "Adagrad", "RowAdagrad"):
        for model in (TRANSE, TRANSH, TRANSD, TRANSR):
            try:
                want = step_plan.plan(**dict(kw, model_id=model, opt_method=opt, counts_supported=int(model == TRANSE)))
            except KgeError:
                continue
            assert want == step_plan.plan(**dict(kw, model_id=model, opt_method=opt, counts_supported=int(model == TRANSE), table_dtype="fp32"))


@pytest.mark.parametrize("change,reason", [
    (dict(model_id=TRANSH, counts_supported=0), "built for TransE only"),
    (dict(model_id=TRANSD, counts_supported=0), "built for TransE only"),
    (dict(model_id=TRANSR, counts_supported=0), "built for TransE only"),
    (dict(counts_supported=0), "needs TransE's sign-count path"),
    (dict(use_counts=False), "needs TransE's sign-count path"),
    (dict(opt_method="Adam"), "needs SGD or RowAdagrad"),
    (dict(opt_method="LazyAdam"), "needs SGD or RowAdagrad"),
    (dict(opt_method="Adagrad"), "needs SGD or RowAdagrad"),
    (dict(width=100), "multiple of 8"),
    (dict(width=20), "multiple of 8"),
    (dict(shared_chunk=8), "cannot be combined with shared negatives"),
    (dict(shared_chunk=8, by_relation=True), "cannot be combined with shared negatives"),
    (dict(bf16_supported=0), "kge_bf16_tables_supported refuses"),
    (dict(table_dtype="fp16"), 'is "fp32" or "bf16"'),
])
def test_refusals_name_the_limit(change, reason):
    with pytest.raises(KgeError) as e:
        step_plan.plan(**dict(BASE, **change))
    assert reason in str(e.value) and ("bf16" in str(e.value))


# ---- the rounding rule ------------------------------------------------------------------------------------------------------------

def test_mix_is_splitmix64s_finaliser():
    """The first outputs of splitmix64 from state 0 are mix(G), mix(2 G), ... (the published test vector)."""
    with np.errstate(over="ignore"):
        got = [int(ref.mix64(ref.GAMMA * np.uint64(i))) for i in (1, 2, 3)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_representable_values_keep_their_bits_for_every_rnd():
    vals = np.array([0.0, -0.0, 1.0, -1.5, 3.140625, 2.0 ** -126, 2.0 ** -133, -2.0 ** -130, 3.3895313892515355e38, -3.3895313892515355e38],
                    np.float32)
    assert (vals.view(np.uint32) & 0xFFFF == 0).all()
    rnd = np.arange(65536, dtype=np.uint32)
    for v in vals:
        got = ref.round_stochastic(np.full(65536, v, np.float32), rnd)
        assert (got == (np.float32(v).view(np.uint32) >> 16)).all(), v


def test_other_values_land_on_one_of_their_two_neighbours():
    rng = np.random.default_rng(5)
    y = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-30, 30, 4000), [1e-40, -3e-39, 1.0000001, -0.3]]).astype(np.float32)
    lo, hi = ref.neighbours(y.astype(np.float64))
    for rnd in (0, 1, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF):
        got = ref.round_stochastic(y, np.full(y.shape, rnd, np.uint32))
        assert ((got == lo) | (got == hi)).all(), rnd
    rnd = rng.integers(0, 65536, y.shape).astype(np.uint32)
    got = ref.round_stochastic(y, rnd)
    assert ((got == lo) | (got == hi)).all()
    assert (ref.round_stochastic(y, np.zeros(y.shape, np.uint32)) == lo).all()      # rnd = 0 truncates


def test_nan_and_inf_are_kept():
    rnd = np.arange(65536, dtype=np.uint32)
    for v, bits in ((np.inf, 0x7F80), (-np.inf, 0xFF80)):
        assert (ref.round_stochastic(np.full(65536, v, np.float32), rnd) == bits).all()
    got = ref.widen(ref.round_stochastic(np.full(65536, np.nan, np.float32), rnd))
    assert np.isnan(got).all()


def test_a_quarter_fraction_rounds_up_in_a_quarter_of_the_draws():
    """One value a quarter of the way between two bf16 values, stored 2^16 times under different (key, column): the share that
    rounds up is within 4 standard deviations of 1/4 (sd = sqrt(1/4 * 3/4 / 2^16) = 1.69e-3)."""
    D, rows = 64, 1024
    y = np.float32(1.0) + np.float32(2.0 ** -9)        # 1 + ulp / 4 (a bf16 ulp at 1.0 is 2^-7)
    assert int(np.float32(y).view(np.uint32)) & 0xFFFF == 0x4000
    got = ref.round_rows(np.full((rows, D), y, np.float32), 1000 + np.arange(rows), seed=12345, step=7)
    up = got == ((np.float32(1.0).view(np.uint32) >> 16) + 1)
    assert (up | (got == (np.float32(1.0).view(np.uint32) >> 16))).all()
    n = rows * D
    assert n == 1 << 16
    assert abs(up.mean() - 0.25) <= 4 * np.sqrt(0.25 * 0.75 / n), up.mean()


def test_the_bits_depend_on_seed_step_key_and_column():
    D = 16
    a = ref.round_bits(1, 0, np.arange(8).reshape(-1, 1), D, np.arange(D).reshape(1, -1))
    assert a.shape == (8, D) and a.max() < 65536
    assert (a != ref.round_bits(2, 0, np.arange(8).reshape(-1, 1), D, np.arange(D).reshape(1, -1))).mean() > 0.99
    assert (a != ref.round_bits(1, 1, np.arange(8).reshape(-1, 1), D, np.arange(D).reshape(1, -1))).mean() > 0.99
    # one mix serves four columns: row key, columns 4c .. 4c + 3 are the four 16-bit fields of one word
    with np.errstate(over="ignore"):
        z = ref.mix64(ref.step_key(1, 0) + ref.GAMMA * np.uint64(3 * (D // 4) + 2 + 1))
    assert [int(x) for x in a[3, 8:12]] == [(int(z) >> (16 * i)) & 0xFFFF for i in range(4)]


def test_round_to_nearest_even_of_table_creation():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.1], np.float32)
    got = ref.widen(ref.to_bf16(x))
    assert list(got[:4]) == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7] and abs(got[4] + 0.1) < 2.0 ** -11


# ---- the driver's switches and the checkpoint record ---------------------------------------------------------------------------

def test_driver_switches():
    from openkeonspark_amd import distribute_training as dt
    a = dt.parse_args([])
    assert a.table_dtype == "fp32" and a.table_rounding_seed == 0
    a = dt.parse_args(["--table_dtype", "bf16", "--table_rounding_seed", "77"])
    assert a.table_dtype == "bf16" and a.table_rounding_seed == 77
    with pytest.raises(SystemExit):
        dt.parse_args(["--table_dtype", "fp16"])


class _Run(object):
    def __init__(self, bf16, seed=0):
        self._bf16, self._table_seed = bf16, seed


def test_checkpoint_record_across_resumes(capsys):
    from openkeonspark_amd import distribute_training as dt
    rec = dt.table_dtype_record(_Run(True, 2 ** 63 + 5))
    assert rec.dtype == np.uint64 and [int(x) for x in rec] == [1, 2 ** 63 + 5]
    dt.check_table_dtype_record({"table_dtype": rec}, _Run(True, 2 ** 63 + 5))          # the same seed resumes
    dt.check_table_dtype_record({"table_dtype": rec}, _Run(False))                     # an fp32 run takes a bf16 checkpoint
    dt.check_table_dtype_record({}, _Run(False))
    assert capsys.readouterr().out == ""
    dt.check_table_dtype_record({}, _Run(True, 3))                                     # a bf16 run takes an fp32 checkpoint, and says so
    assert "rounded to nearest-even once" in capsys.readouterr().out
    with pytest.raises(KgeError) as e:
        dt.check_table_dtype_record({"table_dtype": rec}, _Run(True, 6))
    assert "rounding seed" in str(e.value) and "--table_rounding_seed" in str(e.value)


def test_set_table_dtype_checks_its_arguments():
    import openkeonspark_amd as pkg
    con = pkg.Config.__new__(pkg.Config)      # (no library needed for the setter)
    con.set_table_dtype("bf16", seed=9)
    assert con._bf16 and con._table_seed == 9
    con.set_table_dtype("fp32")
    assert not con._bf16
    for bad in (dict(dtype="fp16"), dict(dtype="bf16", seed=-1), dict(dtype="bf16", seed=2 ** 64)):
        with pytest.raises(KgeError):
            con.set_table_dtype(**bad)
