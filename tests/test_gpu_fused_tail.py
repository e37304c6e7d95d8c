"""The fused single-process TransE step without its closing launch (engine option counts_fused_tail = 1, the default: the last
segapply_kernel team to add into a row of the count image applies that row -- csrc/transe_counts.hip, "the last arrival applies
the row") against the step it replaces (counts_fused_tail = 0: segapply_kernel, then apply_counts_kernel over the image rows) on the
same batches.

The owner calls the same row update on the same integer sums, so everything is compared BIT FOR BIT after three steps (three:
the arrival counters must clean themselves): the loss of every step, both tables, both Adam moments, the emit kernel's 1/|row|
table, the next batch a riding sampler drew, and the count image the step was given, which must be all zero after EVERY step.

Shapes, the smallest that reach each branch: widths 132, 200, 256 (a full wave per team) and 100 (two teams per wave: the ticket
is handed round the team by a shuffle); 1 and 25 negatives; 1, 3, 74 and 513 groups (one group, a partial workgroup, either
side of one 2 048-key sort tile); counts_fused_cap 0 (the default, 64), 1 and 2 (nearly every touched entity row is cut into
pieces: the hub path without a large graph, both lists long or one long and one short); 7 relations (at one group six of them
have no record and still take Adam's decay) and one relation (every relation record on the copies of one row: many arrivals on
one ticket); SGD (untouched rows must not move); a hand-fed batch with a deferred group (residual rows through the owner); the
three-launch sort (its planner counts arrivals too); the sampler riding in the launch that ends the step."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, R, W = 100, 7, 8
NBATCH = 3
MARGIN = 0.5              # random rows: p - score spreads about +-1 around 0, so hinges fall on either side
SEEDS = np.array([1804289383, 846930886, 1681692777, 1714636915, 1957747793, 424238335, 719885386, 1649760492], np.uint64)
DEFAULTS = ((b"counts_fused_tail", 1), (b"counts_fused_cap", 0), (b"counts_sort_tiles", 1), (b"ride_shares", -1))
CLOSING = 100 << 24       # ride_shares: all of an armed sampler in the launch that ends the step


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    for name, v in DEFAULTS:
        L.kge_set_option(name, v)


def graph(n_pos, rels=R):
    """NBATCH * n_pos distinct triples over E entities and `rels` relations: NBATCH batches of n_pos groups."""
    rng = np.random.default_rng(1000 * n_pos + rels)
    seen = set()
    while len(seen) < NBATCH * n_pos:
        seen.add((int(rng.integers(0, E)), int(rng.integers(0, E)), int(rng.integers(0, rels))))
    tri = np.array(sorted(seen), np.int64)
    tri = tri[rng.permutation(len(tri))]
    return E, rels, tri[:, 0], tri[:, 1], tri[:, 2]


def tables(D, seed, rels=R):
    rng = np.random.default_rng(seed)
    return {"ent_embeddings": rng.standard_normal((E, D)).astype(np.float32),
            "rel_embeddings": rng.standard_normal((rels, D)).astype(np.float32)}


def make_config(arrays, n_pos, D, n, params, opt):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.counts_min_records = 0          # these small steps take the sign-count path ...
    con.fused_counts = True             # ... and its fused form
    con.prefetch_sampling = True        # the next batch's sampler rides in the step's launches
    con.set_work_threads(W); con.set_bern(1)
    con.set_dimension(D); con.set_nbatches(NBATCH)
    con.set_ent_neg_rate(n); con.set_rel_neg_rate(0); con.set_margin(MARGIN)
    con.set_opt_method(opt); con.set_alpha(0.001 if opt == "Adam" else 0.01)
    con.init_from_arrays(*arrays)
    con.set_model_and_session(pkg.TransE)
    assert con.batch_size == n_pos and con.use_counts and not con.sparse_rows
    con.set_parameters(params)
    assert con.lib.kge_set_stream_states(SEEDS.ctypes.data, W) == 0
    return con


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def step_keys(L, n_pos, n):
    """The keys of the step just made, slot-major: 2 * virtual row + kind, -1 = no record."""
    keys = np.zeros(n_pos * (3 + n), np.int32)
    assert L.kge_transe_step_scratch_read(1, 0, keys.size, keys.ctypes.data) == 0
    # the doubled key space only the fused step sorts by: the positives' int8 records on even keys, the negatives' 2-bit records on odd ones
    pos, neg = keys[:3 * n_pos], keys[3 * n_pos:]
    assert (pos[pos >= 0] & 1 == 0).all() and (neg[neg >= 0] & 1 == 1).all(), "not the fused step's keys"
    return keys


def run_steps(L, tail, arrays, n_pos, D, n, params, opt="Adam", cap=0, tiles=1, ride=-1, steps=3, fed=None):
    """`steps` steps from the same tables and sampler state -> (per-step results, final state)."""
    import torch
    for name, v in ((b"counts_fused_tail", tail), (b"counts_fused_cap", cap), (b"counts_sort_tiles", tiles), (b"ride_shares", ride)):
        L.kge_set_option(name, v)
    con = make_config(arrays, n_pos, D, n, params, opt)
    per_step = []
    for _ in range(steps):
        loss = con.train_step() if fed is None else con.train_step(fed[0], fed[1], fed[2], None)
        torch.cuda.synchronize()
        assert int(con._counts.abs().max().item()) == 0, "count image not zero after the step"
        per_step.append({"loss": np.float32(loss).tobytes(), "keys": step_keys(L, n_pos, n),
                         "rel": con.get_parameters()["rel_embeddings"].copy()})
    out = {k: v.copy() for k, v in con.get_parameters().items()}
    if opt == "Adam":
        for i, k in enumerate(con.trainModel.table_names):
            out["m/" + k] = con._adam_m[i].cpu().numpy()
            out["v/" + k] = con._adam_v[i].cpu().numpy()
    inv = np.zeros(con.entTotal + con.relTotal, np.float32)
    assert L.kge_transe_step_scratch_read(2, 0, inv.size, inv.ctypes.data) == 0
    out["1/|row|"] = inv
    if fed is None:     # the batch drawn ahead by the sampler that rode in this step
        out["next"] = np.stack([b.cpu().numpy() for b in con._prefetched[0][:3]])
    return per_step, out


def compare(old, new, what):
    assert [s["loss"] for s in old[0]] == [s["loss"] for s in new[0]], what
    for a, b in zip(old[0], new[0]):
        assert np.array_equal(a["keys"], b["keys"]), what
        assert np.array_equal(bits(a["rel"]), bits(b["rel"])), what
    assert set(old[1]) == set(new[1]), what
    for k in old[1]:
        assert np.array_equal(bits(old[1][k]), bits(new[1][k])), (k,) + tuple(what)


def longest_list(keys):
    live = keys[keys >= 0]
    return int(np.bincount(live).max()) if live.size else 0


def touched_rows(per_step, rels):
    """Entity rows and relations with a record in any of the steps."""
    ent, rel = set(), set()
    for s in per_step:
        rows = np.unique(s["keys"][s["keys"] >= 0] >> 1)
        ent.update(int(r) for r in rows[rows < E])
        rel.update(int(r - E) % rels for r in rows[rows >= E])
    return ent, rel


# (n_neg, n_pos, D): every batch size at every width, and the two-teams-per-wave width at the sizes that cut rows
CASES = [(n, n_pos, D) for D in (132, 200, 256) for n in (1, 25) for n_pos in (1, 3, 74, 513)] + [(25, 74, 100), (1, 513, 100)]


@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("n,n_pos,D", CASES)
def test_steps_equal_bit_for_bit(lib, n, n_pos, D, opt):
    arrays = graph(n_pos)
    params = tables(D, 100 * D + n)
    for cap in (0, 1, 2):
        what = (n, n_pos, D, opt, cap)
        old = run_steps(lib, 0, arrays, n_pos, D, n, params, opt=opt, cap=cap)
        new = run_steps(lib, 1, arrays, n_pos, D, n, params, opt=opt, cap=cap)
        compare(old, new, what)
        ent, rel = touched_rows(new[0], R)
        if n == 25 or n_pos >= 74:      # (one negative and a handful of groups: every hinge of the three steps may be idle)
            assert ent and rel, what
            assert not np.array_equal(new[1]["ent_embeddings"], params["ent_embeddings"]), what
            assert not np.array_equal(new[1]["rel_embeddings"], params["rel_embeddings"]), what     # a relation row went through an owner
        if cap and n_pos >= 74:
            assert max(longest_list(s["keys"]) for s in new[0]) > cap, what        # rows were cut into pieces
        if opt == "SGD":        # untouched rows must not move
            idle_e = sorted(set(range(E)) - ent)
            idle_r = sorted(set(range(R)) - rel)
            assert np.array_equal(bits(new[1]["ent_embeddings"][idle_e]), bits(params["ent_embeddings"][idle_e])), what
            assert np.array_equal(bits(new[1]["rel_embeddings"][idle_r]), bits(params["rel_embeddings"][idle_r])), what
            if n_pos <= 3:
                assert idle_e and idle_r, what


def test_record_less_relations_take_the_decay(lib):
    """Three groups per step over seven relations: at least four relations have no record in a step.  Under TF1 Adam a relation
    touched in an earlier step still moves (its moments decay) -- its copy-0 team is the row's only arrival and applies it."""
    n, n_pos, D = 25, 3, 200
    arrays = graph(n_pos)
    params = tables(D, 11)
    old = run_steps(lib, 0, arrays, n_pos, D, n, params)
    new = run_steps(lib, 1, arrays, n_pos, D, n, params)
    compare(old, new, ("record-less relations",))
    moved = 0
    for before, s in zip(new[0][:-1], new[0][1:]):
        _, rel_now = touched_rows([s], R)
        idle = sorted(set(range(R)) - rel_now)
        assert len(idle) >= R - n_pos
        moved += int((bits(before["rel"][idle]) != bits(s["rel"][idle])).any(axis=1).sum())
    assert moved > 0


def test_one_relation(lib):
    """A graph with one relation: every group's relation record falls on the copies of one row, cut into pieces -- many arrivals
    on one ticket, one owner."""
    n, n_pos, D = 25, 74, 200
    arrays = graph(n_pos, rels=1)
    params = tables(D, 77, rels=1)
    for cap in (0, 1, 2):
        old = run_steps(lib, 0, arrays, n_pos, D, n, params, cap=cap)
        new = run_steps(lib, 1, arrays, n_pos, D, n, params, cap=cap)
        compare(old, new, ("one relation", cap))
        assert not np.array_equal(new[1]["rel_embeddings"], params["rel_embeddings"])
        rel_keys = [s["keys"][(s["keys"] >> 1) >= E] for s in new[0]]
        assert max(longest_list(k) for k in rel_keys) > 2          # a relation copy longer than caps 1 and 2: cut into pieces


@pytest.mark.parametrize("tiles", [0, 1])
def test_both_planners_count_arrivals(lib, tiles):
    """The step under the three-launch sort (bkt_sort_kernel) and the two-launch sort (bkt_merge_kernel)."""
    n, n_pos, D = 25, 74, 200
    arrays = graph(n_pos)
    params = tables(D, 13)
    for cap in (0, 2):
        for opt in ("Adam", "SGD"):
            old = run_steps(lib, 0, arrays, n_pos, D, n, params, opt=opt, cap=cap, tiles=tiles)
            new = run_steps(lib, 1, arrays, n_pos, D, n, params, opt=opt, cap=cap, tiles=tiles)
            compare(old, new, ("tiles", tiles, cap, opt))
            assert not np.array_equal(new[1]["rel_embeddings"], params["rel_embeddings"])
            if cap:
                assert longest_list(new[0][-1]["keys"]) > cap


def test_hand_fed_batch_with_a_deferred_group(lib):
    """A fed batch, sampler-shaped but for ONE group whose second negative differs from its positive in two slots: the emit kernel
    defers that group (all S keys -1) and the exact fp32 pass adds its gradient into the residual tables -- its relation row,
    and at cap 2 its entity rows, get those residuals from the row's owner."""
    n, n_pos, D, odd = 25, 74, 200, 41
    rng = np.random.default_rng(3)
    h = rng.integers(0, E, n_pos); t = rng.integers(0, E, n_pos); r = rng.integers(0, R, n_pos)
    H, T, Rr = [h], [t], [r]
    for k in range(n):
        which = rng.integers(0, 2, n_pos)
        nh = np.where(which == 0, (h + 1 + rng.integers(0, E - 1, n_pos)) % E, h)
        nt = np.where(which == 1, (t + 1 + rng.integers(0, E - 1, n_pos)) % E, t)
        if k == 1:
            nh[odd] = (h[odd] + 1) % E; nt[odd] = (t[odd] + 1) % E
        H.append(nh); T.append(nt); Rr.append(r)
    fed = [np.concatenate(x).astype(np.int64) for x in (H, T, Rr)]
    arrays = graph(n_pos)
    params = tables(D, 5)
    for opt in ("Adam", "SGD"):
        for cap in (0, 2):
            got = []
            for tail in (0, 1):
                got.append(run_steps(lib, tail, arrays, n_pos, D, n, params, opt=opt, cap=cap, steps=2, fed=fed))
                deferred = ctypes.c_int32(-1)
                assert lib.kge_transe_deferred_groups(ctypes.byref(deferred)) == 0 and deferred.value == 1
            compare(got[0], got[1], ("hand-fed", opt, cap))
            keys = got[1][0][-1]["keys"].reshape(3 + n, n_pos)
            assert (keys[:, odd] == -1).all()
            others = np.delete(keys, odd, axis=1)
            assert (others[:3] >= 0).any() and (others[3:] >= 0).any()
            assert not np.array_equal(got[1][1]["ent_embeddings"], params["ent_embeddings"])
            assert not np.array_equal(got[1][1]["rel_embeddings"], params["rel_embeddings"])


@pytest.mark.parametrize("n,n_pos", [(25, 74), (1, 513)])
def test_sampler_rides_in_the_closing_launch(lib, n, n_pos):
    """ride_shares = 100 << 24: the whole armed sampler rides in the launch that ends the step -- segapply_kernel now.  The next
    batch and every result must equal those of the default placement and of the apply kernel carrying it."""
    D = 200
    arrays = graph(n_pos)
    params = tables(D, 17)
    for cap in (0, 2):
        base = run_steps(lib, 1, arrays, n_pos, D, n, params, cap=cap)
        ridden = run_steps(lib, 1, arrays, n_pos, D, n, params, cap=cap, ride=CLOSING)
        before = run_steps(lib, 0, arrays, n_pos, D, n, params, cap=cap, ride=CLOSING)
        compare(base, ridden, ("ride", n, n_pos, cap))
        compare(before, ridden, ("ride, against the apply kernel", n, n_pos, cap))
        assert ridden[1]["next"].shape == (3, n_pos * (1 + n))
        assert (ridden[1]["next"] >= 0).all() and ridden[1]["next"][:2].max() < E and ridden[1]["next"][2].max() < R
