"""Type-constrained negative sampling on the device (kge_set_typed_sampling, Config.set_type_constrained_sampling) against the
Python restatement of the draw in typed_sampler_cases.py, bit for bit, on a crafted graph that holds every edge case of the
typed pick and on kg_tiny; and what follows from the draw: the untyped batch's positives, coins, relation negatives and stream
states, thread ranges, the armed (prefetch) path, the packed negatives, the persistent-launch rules and the command line."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from openkeonspark_amd import _lib

import typed_sampler_cases as tc

pytestmark = pytest.mark.gpu

SEEDS8 = np.array([1804289383, 846930886, 1681692777, 1714636915, 1957747793, 424238335, 719885386, 1649760492], np.uint64)
SHAPES = tc.GRID_SHAPE + [tc.WIDE_SHAPE]


@pytest.fixture(scope="module")
def kgs(tmp_path_factory):
    return {"crafted": tc.write_crafted(str(tmp_path_factory.mktemp("kg_typed_crafted"))),
            "tiny": tc.KG(os.path.join(GOLDEN, "kg_tiny"))}


@pytest.fixture(autouse=True)
def typed_off_afterwards():
    yield
    L = _lib.lib()
    L.kge_set_typed_sampling(0)
    L.kge_set_option(b"emit_pack", 1)
    L.kge_clear_error()


def make_config(path, W, bern, typed=True, **attrs):
    from openkeonspark_amd.Config import Config
    con = Config()
    for k, v in attrs.items():
        setattr(con, k, v)
    con.set_in_path(path)
    con.set_work_threads(W)
    con.set_bern(bern)
    con.set_type_constrained_sampling(typed)
    return con


def set_states(con, seeds):
    seeds = np.ascontiguousarray(seeds, np.uint64)
    assert con.lib.kge_set_stream_states(seeds.ctypes.data, len(seeds)) == 0


def abi_sampling(con, B, n, nr):
    tot = B * (1 + n + nr)
    h, t, r = (np.zeros(tot, np.int64) for _ in range(3))
    y = np.zeros(tot, np.float32)
    con.lib.kge_clear_error()
    con.lib.sampling(h.ctypes.data, t.ctypes.data, r.ctypes.data, y.ctypes.data, B, n, nr)
    _lib.raise_if_error(con.lib)
    assert (y[:B] == 1).all() and (y[B:] == -1).all()
    return h, t, r


def device_run(con, seeds):
    """Every shape, three calls each, through the Base.so-compatible `sampling`: the batches and the final states."""
    set_states(con, seeds)
    out = [abi_sampling(con, B, n, nr) for (B, n, nr) in SHAPES for _ in range(tc.CALLS)]
    return out, [int(x) for x in con.get_stream_states()]


def restated_run(kg, seeds, bern, typed):
    states = [int(x) for x in seeds]
    out = [tc.sample_batch(kg, states, B, n, nr, bern, typed) for (B, n, nr) in SHAPES for _ in range(tc.CALLS)]
    return out, states


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("bern", [0, 1])
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("which", ["crafted", "tiny"])
def test_typed_batches_equal_the_restatement_bit_for_bit(kgs, which, W, bern):
    kg = kgs[which]
    seeds = SEEDS8[:W]
    con = make_config(kg.path, W, bern)
    con.init()
    assert con.lib.kge_typed_sampling() == 1
    got, got_states = device_run(con, seeds)
    want, want_states = restated_run(kg, seeds, bern, typed=True)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (SHAPES[i // tc.CALLS], i % tc.CALLS)
    assert got_states == want_states
    # the stream states are those of an untyped run from the same seeds, on the device too; and the mode did change batches
    con.set_type_constrained_sampling(False)
    plain, plain_states = device_run(con, seeds)
    assert plain_states == got_states
    assert any(not same(g, p) for g, p in zip(got, plain))


@pytest.mark.parametrize("which", ["crafted", "tiny"])
def test_typed_batch_agrees_with_the_untyped_batch_from_the_same_states(kgs, which):
    kg = kgs[which]
    W, bern = 3, 1
    con = make_config(kg.path, W, bern)
    con.init()
    typed, _ = device_run(con, SEEDS8[:W])
    con.set_type_constrained_sampling(False)
    plain, _ = device_run(con, SEEDS8[:W])
    restated, _ = restated_run(kg, SEEDS8[:W], bern, typed=True)
    n_typed = n_fallback = 0
    for i, (B, n, nr) in enumerate(s for s in SHAPES for _ in range(tc.CALLS)):
        (th, tt, tr), (ph, pt, pr), info = typed[i], plain[i], restated[i][3]
        assert same(typed[i], restated[i])
        assert np.array_equal(th[:B], ph[:B]) and np.array_equal(tt[:B], pt[:B]) and np.array_equal(tr[:B], pr[:B])     # positives
        ent = slice(B, B * (1 + n))
        pos_t, pos_h = np.tile(tt[:B], n), np.tile(th[:B], n)
        # an entity negative changes exactly the side the coin chose, in both modes, and keeps the relation
        assert np.array_equal(tt[ent] != pos_t, pt[ent] != pos_t) and np.array_equal(th[ent] != pos_h, ph[ent] != pos_h)
        assert ((tt[ent] != pos_t) ^ (th[ent] != pos_h)).all()
        assert np.array_equal(tr[ent], pr[ent]) and np.array_equal(tr[ent], np.tile(tr[:B], n))
        rel = slice(B * (1 + n), None)                              # relation negatives: untouched
        assert np.array_equal(th[rel], ph[rel]) and np.array_equal(tt[rel], pt[rel]) and np.array_equal(tr[rel], pr[rel])
        for (b, k), (new_tail, in_list) in info.items():
            o = b + k * B
            h, t, r = int(th[o]), int(tt[o]), int(tr[o])
            assert (t != int(tt[b])) == new_tail
            if in_list:
                n_typed += 1
                assert (t in kg.tail_list[r]) if new_tail else (h in kg.head_list[r])
                assert (h, t, r) not in kg.uniq
            else:
                n_fallback += 1
                assert (h, t, r) == (int(ph[o]), int(pt[o]), int(pr[o]))       # the reference's draw from the same s
    assert n_typed > 0 and (n_fallback > 0 or which == "tiny")


def test_switching_off_again_reproduces_the_reference_fixture(kgs):
    W, bern = 2, 1
    z = np.load(os.path.join(GOLDEN, "kg_tiny_W%d_bern%d.npz" % (W, bern)))
    con = make_config(kgs["tiny"].path, W, bern)
    con.init()
    set_states(con, z["seeds"])
    abi_sampling(con, 64, 2, 1)
    con.set_type_constrained_sampling(False)
    assert con.lib.kge_typed_sampling() == 0
    set_states(con, z["seeds"])
    for si, (B, n, nr) in enumerate(tc.GRID_SHAPE):
        for c in range(tc.CALLS):
            h, t, r = abi_sampling(con, B, n, nr)
            ref = z["s%d_c%d" % (si, c)]
            assert np.array_equal(h, ref[0]) and np.array_equal(t, ref[1]) and np.array_equal(r, ref[2]), (si, c)
    assert con.get_stream_states().tolist() == z["final_states"].tolist()


@pytest.mark.parametrize("shape", [(50, 3, 1), tc.WIDE_SHAPE])
def test_thread_ranges_of_ranks_union_to_the_typed_batch(kgs, shape):
    import torch
    kg = kgs["crafted"]
    W, bern = 8, 1
    B, n, nr = shape
    con = make_config(kg.path, W, bern)
    con.init()
    for G in (1, 2, 4):
        states = [int(x) for x in SEEDS8]
        set_states(con, SEEDS8)
        for call in range(2):
            before = np.array(states, np.uint64)
            want = tc.sample_batch(kg, states, B, n, nr, bern, typed=True)
            got = [np.zeros_like(want[0]) for _ in range(3)]
            for g in range(G):
                set_states(con, before)                      # every rank starts from the same states
                lo, hi = g * W // G, (g + 1) * W // G
                first = ctypes.c_int64()
                cnt = con.lib.kge_slice_positions(B, lo, hi, ctypes.byref(first))
                stride = max(cnt, 1)
                buf = torch.zeros((3, stride * (1 + n + nr)), dtype=torch.int32, device="cuda")
                nl = ctypes.c_int64()
                rc = con.lib.kge_sampling_device(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), B, n, nr, lo, hi, stride,
                                                 ctypes.byref(nl), None)
                assert rc == 0 and nl.value == cnt
                host = buf.cpu().numpy()
                for k in range(1 + n + nr):
                    for a in range(3):
                        got[a][k * B + first.value:k * B + first.value + cnt] = host[a][k * stride:k * stride + cnt]
            assert same(got, want), (G, call)
            assert [int(x) for x in con.get_stream_states()] == states


def test_armed_sampler_draws_the_same_sequence_as_direct_sampling(kgs):
    """kge_sampling_attach + kge_sampling_flush (what a step with prefetch_sampling does) against kge_sampling_device, typed."""
    import torch
    kg = kgs["crafted"]
    W, bern, (B, n, nr) = 3, 1, (50, 3, 1)
    con = make_config(kg.path, W, bern)
    con.init()
    slots = 1 + n + nr
    states = [int(x) for x in SEEDS8[:W]]
    want = [tc.sample_batch(kg, states, B, n, nr, bern, typed=True) for _ in range(4)]

    def draw(armed):
        set_states(con, SEEDS8[:W])
        out = []
        for i in range(4):
            buf = torch.zeros((3, B * slots), dtype=torch.int32, device="cuda")
            nl = ctypes.c_int64()
            fn = con.lib.kge_sampling_attach if (armed and i % 2 == 0) else con.lib.kge_sampling_device     # (armed, direct, armed, direct)
            assert fn(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), B, n, nr, 0, W, B, ctypes.byref(nl), None) == 0
            out.append(buf)
        assert con.lib.kge_sampling_flush(None) == 0
        torch.cuda.synchronize()
        return [b.cpu().numpy().astype(np.int64) for b in out], [int(x) for x in con.get_stream_states()]

    direct, s_direct = draw(False)
    armed, s_armed = draw(True)
    for i in range(4):
        assert same(direct[i], want[i]) and same(armed[i], want[i]), i
    assert s_direct == s_armed == states


def train_config(kg, model_name, typed, prefetch, D, n, nbatches, opt="SGD", alpha=0.01, **attrs):
    import openkeonspark_amd as pkg
    con = make_config(kg.path, 8, 1, typed=typed, prefetch_sampling=prefetch, **attrs)
    con.set_dimension(D); con.set_nbatches(nbatches); con.set_ent_neg_rate(n); con.set_margin(1.0)
    con.set_opt_method(opt); con.set_alpha(alpha)
    con.seed = 11
    con.init()
    con.set_model_and_session(getattr(pkg, model_name))
    set_states(con, SEEDS8)
    return con


def losses_and_tables(con, steps):
    import torch
    losses = [np.float32(con.train_step()).tobytes() for _ in range(steps)]
    torch.cuda.synchronize()
    return losses, {k: v.copy() for k, v in con.get_parameters().items()}


def equal_runs(a, b):
    return a[0] == b[0] and all(np.array_equal(a[1][k].view(np.uint32), b[1][k].view(np.uint32)) for k in a[1])


def test_steps_with_prefetch_equal_steps_without(kgs):
    """sample_device / attach / flush inside train_step: the typed sampler armed by a step (it rides nowhere, the flush launches
    it) draws the batches direct sampling draws.  TransE on the sign-count path: its integer sums make a run reproducible bit
    for bit, so equal batches give equal bits."""
    def run(typed, prefetch):
        return losses_and_tables(train_config(kgs["tiny"], "TransE", typed, prefetch, 64, 3, 2, counts_min_records=0), 4)
    runs = [run(True, prefetch) for prefetch in (False, True)]
    assert runs[0][0] == runs[1][0]
    assert equal_runs(*runs)
    assert not equal_runs(runs[0], run(False, False))


def test_packed_negatives_agree_with_the_ids(kgs):
    """TransE on the sign-count path, typed: the step that reads the sampler's packed line against the step that reads the ids."""
    runs = []
    for pack in (0, 1):
        _lib.lib().kge_set_option(b"emit_pack", pack)
        con = train_config(kgs["tiny"], "TransE", True, True, 132, 25, 2, counts_min_records=0)
        assert con.use_counts and not con.sparse_rows and con.lib.kge_typed_sampling() == 1
        runs.append(losses_and_tables(con, 3))
        assert (con._dev_pack is not None) == bool(pack)
    assert equal_runs(*runs)


def test_a_short_typed_transh_run_trains(kgs):
    con = train_config(kgs["tiny"], "TransH", True, None, 32, 5, 1, alpha=0.05)
    losses = np.array([con.train_step() for _ in range(60)], np.float64)
    assert np.isfinite(losses).all()
    assert losses[-10:].mean() < losses[:10].mean()


def test_persistent_launch_is_off_in_typed_mode(kgs):
    from openkeonspark_amd.Config import KgeError
    con = train_config(kgs["tiny"], "TransE", True, False, 32, 2, 2)
    assert not con.persistent_supported() and not con.persistent_preferred()
    con.type_constrained_sampling = False
    assert con.persistent_supported()            # the typed mode is the only reason
    con.type_constrained_sampling = True
    with pytest.raises(KgeError, match="type-constrained"):
        con.train_steps(3, persistent=True)
    # launched steps, on the sign-count path (integer sums: reproducible bit for bit)
    con2 = train_config(kgs["tiny"], "TransE", True, False, 32, 2, 2, counts_min_records=0)
    many = con2.train_steps(5)
    tables = {k: v.copy() for k, v in con2.get_parameters().items()}
    ref = train_config(kgs["tiny"], "TransE", True, False, 32, 2, 2, counts_min_records=0)
    one_by_one = losses_and_tables(ref, 5)
    assert [np.float32(x).tobytes() for x in many] == one_by_one[0]
    assert all(np.array_equal(tables[k].view(np.uint32), one_by_one[1][k].view(np.uint32)) for k in tables)
    # the C entry point refuses as well
    lr = np.full(1, 0.01, np.float32)
    import torch
    out = torch.zeros(1, device="cuda")
    rc = con.lib.kge_train_steps_persistent(ctypes.byref(con._desc), con._tab_ptrs, con._grad_ptrs, None, None, con.batch_size, 2, 0, 1, 0,
                                            lr.ctypes.data, 0.9, 0.999, 1e-8, out.data_ptr(), None)
    assert rc < 0 and "type-constrained" in _lib.last_error(con.lib)
    con.lib.kge_clear_error()


def test_sampler_kernel_timer(kgs):
    """Engine option time_sampler and the kernel name "sampler" of kge_last_kernel_ms / kge_kernel_ms_mean (what
    tools/typed_sampler_cost.py reads): every launch of the sampler's own kernels is bracketed, typed or not."""
    con = make_config(kgs["crafted"].path, 3, 1)
    con.init()
    L = con.lib
    ms, n = ctypes.c_float(-1), ctypes.c_int64(-1)
    try:
        assert L.kge_set_option(b"time_sampler", 1) == 0
        assert L.kge_kernel_ms_mean(b"sampler", ctypes.byref(ms), ctypes.byref(n)) < 0      # nothing launched yet
        L.kge_clear_error()
        for typed in (True, False, True):
            con.set_type_constrained_sampling(typed)
            abi_sampling(con, 50, 3, 1)
        assert L.kge_kernel_ms_mean(b"sampler", ctypes.byref(ms), ctypes.byref(n)) == 0
        assert n.value == 3 and 0 < ms.value < 100
        last = ctypes.c_float(-1)
        assert L.kge_last_kernel_ms(b"sampler", ctypes.byref(last)) == 0 and 0 < last.value < 100
        assert L.kge_kernel_ms_mean(b"no_such_kernel", ctypes.byref(ms), ctypes.byref(n)) < 0
        L.kge_clear_error()
    finally:
        L.kge_set_option(b"time_sampler", 0)


def test_link_prediction_imports_keep_typed_sampling_working(kgs):
    """init_link_prediction() after init(): importTestFiles drops the type lists, Config imports them again for the sampler."""
    kg = kgs["tiny"]
    con = make_config(kg.path, 3, 0)
    con.init()
    con.init_link_prediction()
    assert con.lib.kge_typed_sampling() == 1
    set_states(con, SEEDS8[:3])
    states = [int(x) for x in SEEDS8[:3]]
    assert same(abi_sampling(con, 50, 3, 0), tc.sample_batch(kg, states, 50, 3, 0, 0, typed=True))


def test_command_line_flag_reaches_the_engine(kgs):
    from openkeonspark_amd.distribute_training import get_conf, parse_args
    assert parse_args([]).type_constrained_sampling == 0
    args = parse_args(["--input_path", kgs["crafted"].path, "--type_constrained_sampling", "1", "--n_mini_batches", "2"])
    con = get_conf(args)
    assert con.type_constrained_sampling is True and con.lib.kge_typed_sampling() == 1
    con = get_conf(parse_args(["--input_path", kgs["crafted"].path, "--n_mini_batches", "2"]))
    assert con.type_constrained_sampling is False and con.lib.kge_typed_sampling() == 0
