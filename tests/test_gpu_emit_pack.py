"""The sampler's packed negatives (csrc/sampler_dev.hpp SamplerArgs::pack, engine option emit_pack = 1, the default) and the
TransE round body that reads a group's negatives from them (csrc/models.hip transe_emit_rounds_body<.., PACK>).

The pack is a second description of ids the sampler already writes to the h / t / r arrays, and the emit kernel does the same
arithmetic in the same order whichever of the two it reads.  So every check here is exact: the pack against a numpy rebuild from
the arrays of the same launch, and the training step with the pack against the step without it (emit_pack = 0, which writes,
reads and allocates none) bit for bit -- loss, tables, Adam moments, destination keys, int8 and 2-bit records.

Graph: 100 entities, 7 relations, 390 triples; (head 0, relation 0) has eight known tails and (tail 1, relation 1) eight known
heads, so the sampler's filtered pick also takes its search path (more than four known ids).

Step cases: D = 132 / 200 / 256 (33 / 50 / 64 live lanes) x n = 3 / 25 / 63 / 20 + 5 relation negatives are the twelve
parametrised cases; the eight combinations of {Adam, SGD} x {fused step, two calls} x {prefetch on, off} rotate through them,
two per case, so each combination runs at three different (D, n) and every (D, n) runs two of them."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, R, TRAIN, W = 100, 7, 390, 8
B_STEP = 130              # TRAIN / 3 batches: 33 workgroups of four groups, the last one ragged
MARGIN = 0.5              # random rows: p - score spreads about +-1 around 0, so hinges fall on either side
SEEDS = np.array([1804289383, 846930886, 1681692777, 1714636915, 1957747793, 424238335, 719885386, 1649760492], np.uint64)


@pytest.fixture(scope="module")
def kg_dir(tmp_path_factory):
    from openkeonspark_amd.synthetic import write_openke_dir
    rng = np.random.default_rng(6)
    seen = {(0, t, 0) for t in range(1, 9)} | {(h, 1, 1) for h in range(2, 10)}
    while len(seen) < TRAIN:
        seen.add((int(rng.integers(0, E)), int(rng.integers(0, E)), int(rng.integers(0, R))))
    tri = np.array(sorted(seen), np.int64)
    tri = tri[rng.permutation(len(tri))]
    path = str(tmp_path_factory.mktemp("emit_pack_kg")) + "/"
    write_openke_dir(path, E, R, tri[:, 0], tri[:, 1], tri[:, 2])
    return path


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    L.kge_set_option(b"emit_pack", 1)


def make_config(path, D, n, nr, opt="SGD", model=True, fused=True, prefetch=False, params=None):
    from openkeonspark_amd.Config import Config
    import openkeonspark_amd as pkg
    con = Config()
    con.counts_min_records = 0          # these small steps take the sign-count path
    con.fused_counts = fused
    con.prefetch_sampling = prefetch
    con.set_in_path(path); con.set_work_threads(W); con.set_bern(1)
    con.set_dimension(D); con.set_nbatches(TRAIN // B_STEP)
    con.set_ent_neg_rate(n); con.set_rel_neg_rate(nr); con.set_margin(MARGIN)
    con.set_opt_method(opt); con.set_alpha(0.001 if opt == "Adam" else 0.01)
    con.init()
    if model:
        con.set_model_and_session(pkg.TransE)
        assert con.batch_size == B_STEP and con.use_counts and not con.sparse_rows
        if params is not None:
            con.set_parameters(params)
    assert con.lib.kge_set_stream_states(SEEDS.ctypes.data, W) == 0
    return con


def expected_pack(host, n_pos, stride, slots, kshift):
    """The pack rebuilt from the arrays one sampler launch wrote: [n_pos << kshift] words."""
    want = np.zeros((n_pos, 1 << kshift), np.int64)
    h, t, r = (host[a][:n_pos].astype(np.int64) for a in range(3))
    for k in range(1, slots):
        nh, nt, nr = (host[a][k * stride:k * stride + n_pos].astype(np.int64) for a in range(3))
        code = np.where(nh != h, 0, np.where(nt != t, 1, 2))
        row = np.where(code == 0, nh, np.where(code == 1, nt, nr))
        differ = (nh != h).astype(int) + (nt != t).astype(int) + (nr != r).astype(int)
        want[:, k] = row | (code << 28) | np.where(differ == 1, 0, 1 << 31)
    return want.reshape(-1).astype(np.uint32).view(np.int32)


def kshift_of(slots):
    k = 0
    while (1 << k) < slots:
        k += 1
    return k


NEG_CASES = [(1, 0), (3, 2), (25, 0), (31, 0), (32, 0), (63, 0)]       # kshift 1, 3, 5, 5 (no padding), 6, 6 (no padding)


@pytest.mark.parametrize("n,nr", NEG_CASES)
def test_pack_equals_the_arrays_of_the_same_launch(lib, kg_dir, n, nr):
    """kge_sampling_device_packed over whole batches, a rank's thread range and an empty range: every live word, the zero words
    of slot 0 and of the padding, and nothing written past the pack."""
    import torch
    con = make_config(kg_dir, 200, n, nr, model=False)
    slots = 1 + n + nr
    ks = kshift_of(slots)
    assert ks == {2: 1, 6: 3, 26: 5, 32: 5, 33: 6, 64: 6}[slots]
    live_words = empty_seen = 0
    for Bq in (1, 37, 130):          # two positives in a wave (kshift <= 5), a ragged last wave, several workgroups
        for lo, hi in ((0, W), (2, 4)):      # the whole batch; rank 1 of a 2-of-8 split (B = 1: its slice is empty)
            first = ctypes.c_int64()
            cnt = int(lib.kge_slice_positions(Bq, lo, hi, ctypes.byref(first)))
            stride = max(cnt, 1)
            words = int(lib.kge_emit_pack_words(cnt, n, nr, 200))
            assert words == (cnt << ks)
            buf = torch.full((3, stride * slots), -5, dtype=torch.int32, device="cuda")
            pack = torch.full((words + 64,), -7, dtype=torch.int32, device="cuda")
            nl = ctypes.c_int64()
            rc = lib.kge_sampling_device_packed(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), pack.data_ptr(), Bq, n, nr,
                                                lo, hi, stride, ctypes.byref(nl), None)
            assert rc == 0 and nl.value == cnt
            torch.cuda.synchronize()
            got = pack.cpu().numpy()
            assert (got[words:] == -7).all(), (Bq, lo, hi)
            if cnt == 0:
                empty_seen += 1
                continue
            want = expected_pack(buf.cpu().numpy(), cnt, stride, slots, ks)
            assert np.array_equal(got[:words], want), (Bq, lo, hi)
            grid = got[:words].reshape(cnt, 1 << ks)
            assert (grid[:, 0] == 0).all() and (grid[:, slots:] == 0).all()
            assert (grid[:, 1:slots] >= 0).all()                        # the sampler draws single-slot corruptions only
            live_words += cnt * (slots - 1)
            if nr:
                assert ((grid[:, 1 + n:slots] >> 28) == 2).all()        # relation negatives
    assert empty_seen == 1 and live_words > 0


def test_option_off_writes_no_pack(lib, kg_dir):
    import torch
    con = make_config(kg_dir, 200, 25, 0, model=False)
    lib.kge_set_option(b"emit_pack", 0)
    assert lib.kge_emit_pack_words(37, 25, 0, 200) == 0
    buf = torch.zeros((3, 37 * 26), dtype=torch.int32, device="cuda")
    pack = torch.full((37 << 5,), -7, dtype=torch.int32, device="cuda")
    assert lib.kge_sampling_device_packed(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), pack.data_ptr(), 37, 25, 0, 0, W,
                                          37, None, None) == 0
    torch.cuda.synchronize()
    assert (pack.cpu().numpy() == -7).all()
    lib.kge_set_option(b"emit_pack", 1)
    assert lib.kge_emit_pack_words(37, 25, 0, 200) == 37 << 5
    assert lib.kge_emit_pack_words(37, 64, 0, 200) == 0                 # more than 64 slots: the wide sampler takes no pack
    assert lib.kge_emit_pack_words(37, 25, 0, 100) == 0 and lib.kge_emit_pack_words(37, 25, 0, 130) == 0   # widths outside the round body
    assert lib.kge_emit_pack_words(37, 25, 0, 132) == lib.kge_emit_pack_words(37, 25, 0, 256) == lib.kge_emit_pack_words(37, 25, 0, 0) == 37 << 5


def tables(D, seed):
    rng = np.random.default_rng(seed)
    return {"ent_embeddings": rng.standard_normal((E, D)).astype(np.float32),
            "rel_embeddings": rng.standard_normal((R, D)).astype(np.float32)}


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def run_steps(L, pack, path, D, n, nr, opt, fused, prefetch, params, records=True):
    """Three train_step() on device-sampled batches from fixed tables and rng states -> loss bits, tables, moments, the last step's
    keys and records."""
    import torch
    L.kge_set_option(b"emit_pack", pack)
    con = make_config(path, D, n, nr, opt=opt, fused=fused, prefetch=prefetch, params=params)
    losses = [np.float32(con.train_step()).tobytes() for _ in range(3)]
    torch.cuda.synchronize()
    used = con._dev_pack is not None
    out = {k: v.copy() for k, v in con.get_parameters().items()}
    if opt == "Adam":
        for i, k in enumerate(con.trainModel.table_names):
            out["m/" + k] = con._adam_m[i].cpu().numpy()
            out["v/" + k] = con._adam_v[i].cpu().numpy()
    nn = n + nr
    M, dw = B_STEP * (3 + nn), int(L.kge_transe_record_dwords(ctypes.byref(con._desc)))
    keys = np.zeros(M, np.int32)
    assert L.kge_transe_step_scratch_read(1, 0, M, keys.ctypes.data) == 0
    rec8 = rec2 = None
    if records:
        rec8 = np.zeros(((3 if fused else 3 + nn) * B_STEP, dw), np.uint32)
        assert L.kge_transe_step_scratch_read(0, 0, rec8.size, rec8.ctypes.data) == 0
        if fused:
            rec2 = np.zeros((nn * B_STEP, dw), np.uint8)                # dw bytes per 2-bit record: one per lane
            assert L.kge_transe_step_scratch_read(0, rec8.size, rec2.size // 4, rec2.ctypes.data) == 0
    # the batch drawn ahead by the sampler that rode in the last step, and its pack
    ahead = None
    if prefetch:
        buf, n_pos, _ = con._prefetched
        ahead = (buf.cpu().numpy(), n_pos, con._dev_pack[con._slot].cpu().numpy() if used else None)
    return dict(losses=losses, state=out, keys=keys, rec8=rec8, rec2=rec2, used=used, ahead=ahead)


COMBOS = [(opt, fused, prefetch) for opt in ("Adam", "SGD") for fused in (True, False) for prefetch in (True, False)]
STEP_CASES = [(D, n, nr) for D in (132, 200, 256) for n, nr in ((3, 0), (25, 0), (63, 0), (20, 5))]


def compare(old, new, what):
    assert old["losses"] == new["losses"], what
    for k in old["state"]:
        assert np.array_equal(bits(old["state"][k]), bits(new["state"][k])), (k,) + what
    assert np.array_equal(old["keys"], new["keys"]), what


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_steps_equal_bit_for_bit(lib, kg_dir, case):
    D, n, nr = STEP_CASES[case]
    params = tables(D, 100 * D + n)
    for opt, fused, prefetch in (COMBOS[(2 * case) % 8], COMBOS[(2 * case + 1) % 8]):
        what = (D, n, nr, opt, fused, prefetch)
        old = run_steps(lib, 0, kg_dir, D, n, nr, opt, fused, prefetch, params)
        new = run_steps(lib, 1, kg_dir, D, n, nr, opt, fused, prefetch, params)
        assert new["used"] and not old["used"], what                     # emit_pack = 0 allocates none
        compare(old, new, what)
        assert not np.array_equal(new["state"]["ent_embeddings"], params["ent_embeddings"])
        ko, nn = old["keys"], n + nr
        rows = E + R
        live = (ko >= 0) & (ko < (2 * rows if fused else rows))          # fused: keys are 2 * row + kind
        pos_live, neg_live = live[:3 * B_STEP], live[3 * B_STEP:]
        assert neg_live.any() and not neg_live.all(), what               # active and idle hinges
        if fused:
            assert np.array_equal(old["rec8"][pos_live], new["rec8"][pos_live]), what
            assert np.array_equal(old["rec2"][neg_live][:, :D // 4], new["rec2"][neg_live][:, :D // 4]), what
            assert new["rec2"][neg_live][:, :D // 4].any()
        else:
            assert np.array_equal(old["rec8"][live][:, :D // 4], new["rec8"][live][:, :D // 4]), what
            assert new["rec8"][live][:, :D // 4].any()
        if prefetch:     # the armed sampler that rode in the step drew the same next batch, and its pack describes that batch
            ho, po, _ = old["ahead"]
            hn, pn, pack = new["ahead"]
            assert po == pn == B_STEP and np.array_equal(ho, hn), what
            ks = kshift_of(1 + nn)
            assert np.array_equal(pack, expected_pack(hn, pn, B_STEP, 1 + nn, ks)), what


@pytest.mark.parametrize("D", [100, 64])
def test_other_widths_do_not_change(lib, kg_dir, D):
    """Widths outside the round body: the option changes nothing."""
    params = tables(D, D)
    for opt, fused, prefetch in (("Adam", True, True), ("SGD", False, False)):
        old = run_steps(lib, 0, kg_dir, D, 25, 0, opt, fused, prefetch, params, records=False)
        new = run_steps(lib, 1, kg_dir, D, 25, 0, opt, fused, prefetch, params, records=False)
        compare(old, new, (D, opt, fused, prefetch))
        assert not new["used"] and (old["keys"] >= 0).any()              # no pack is even allocated at these widths


def hand_batch(rng, n):
    """A sampler-shaped batch that is NOT the one the sampler drew: [3, B_STEP * (1 + n)] ids, single-slot entity corruptions."""
    h = rng.integers(0, E, B_STEP); t = rng.integers(0, E, B_STEP); r = rng.integers(0, R, B_STEP)
    H, T, Rr = [h], [t], [r]
    for _ in range(n):
        which = rng.integers(0, 2, B_STEP)
        H.append(np.where(which == 0, (h + 1 + rng.integers(0, E - 1, B_STEP)) % E, h))
        T.append(np.where(which == 1, (t + 1 + rng.integers(0, E - 1, B_STEP)) % E, t))
        Rr.append(r)
    return [np.concatenate(x).astype(np.int64) for x in (H, T, Rr)]


@pytest.mark.parametrize("prefetch", [False, True])
def test_hand_fed_batch_ignores_the_pack_of_a_sampled_step(lib, kg_dir, prefetch):
    """A fed batch after a sampled step on the same engine == the same feed on a fresh emit_pack = 0 engine: the pack left by the
    sampled step (and, with prefetch, the one of the batch drawn ahead) describes other negatives and must not be read."""
    D, n = 200, 25
    h, t, r = hand_batch(np.random.default_rng(44), n)
    lib.kge_set_option(b"emit_pack", 1)
    a = make_config(kg_dir, D, n, 0, prefetch=prefetch, params=tables(D, 9))
    a.train_step()
    assert a._dev_pack is not None
    mid = {k: v.copy() for k, v in a.get_parameters().items()}
    loss_a = a.train_step(h, t, r, None)
    end_a = {k: v.copy() for k, v in a.get_parameters().items()}
    lib.kge_set_option(b"emit_pack", 0)
    b = make_config(kg_dir, D, n, 0, prefetch=prefetch, params=mid)
    loss_b = b.train_step(h, t, r, None)
    assert b._dev_pack is None
    assert np.float32(loss_a).tobytes() == np.float32(loss_b).tobytes()
    for k, v in b.get_parameters().items():
        assert np.array_equal(bits(v), bits(end_a[k])), k
        assert not np.array_equal(v, mid[k]), k
