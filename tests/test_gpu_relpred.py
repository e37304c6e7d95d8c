"""Relation prediction on the device (Config.top_k_relations / relation_prediction, kge_topk_relations /
kge_relation_prediction): scores and order against the predict op called once per relation (so TransR uses each relation's
own matrix), the filter and type constraint against masks built from the dataset files, the four rank counts against a NumPy
brute force, chunking, ties and NaN, no interference with training, argument errors, device tensors, the test() / driver /
two-rank interface and a metric sanity check on a learnable graph.  test_relation_metric_reduction runs without a GPU."""
import json
import os
import shutil
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

gpu = pytest.mark.gpu
KG = os.path.join(GOLDEN, "kg_small")


def make_config(model="TransE", dim=32, path=KG, scale=3.0, test_files=True):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(path)
    con.set_work_threads(1)
    con.set_dimension(dim)
    con.set_test_link_prediction(test_files)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    if scale != 1.0:
        for t in con._tables:      # spread the scores: xavier-initialised tables rank almost at random
            t.mul_(scale)
        con.tables_changed()
    return con


def read_triples(path, name):
    a = np.loadtxt(os.path.join(path, name), dtype=np.int64, skiprows=1, ndmin=2)
    return a[:, 0], a[:, 1], a[:, 2]     # h, t, r


def sorted_test_triples(path):
    """test2id.txt in the library's (r, h, t) order, the order kge_relation_prediction's [first, first + count) indexes."""
    h, t, r = read_triples(path, "test2id.txt")
    o = np.lexsort((t, h, r))
    return h[o], t[o], r[o]


def known_set(path):
    known = set()
    for name in ("train2id.txt", "valid2id.txt", "test2id.txt"):
        h, t, r = read_triples(path, name)
        known.update(zip(h.tolist(), t.tolist(), r.tolist()))
    return known


def type_lists(path, R):
    heads, tails = [set() for _ in range(R)], [set() for _ in range(R)]
    with open(os.path.join(path, "type_constrain.txt")) as f:
        lines = f.read().split("\n")[1:]
    for i in range(R):
        hl, tl = lines[2 * i].split(), lines[2 * i + 1].split()
        heads[int(hl[0])].update(int(x) for x in hl[2:])
        tails[int(tl[0])].update(int(x) for x in tl[2:])
    return heads, tails


def masks(path, h, t, R, filtered, typed):
    """eligible[i, r]: relation r may be returned for (h_i, ?, t_i)"""
    ok = np.ones((len(h), R), bool)
    if filtered:
        known = known_set(path)
        for i in range(len(h)):
            for r in range(R):
                if (int(h[i]), int(t[i]), r) in known:
                    ok[i, r] = False
    if typed:
        heads, tails = type_lists(path, R)
        for i in range(len(h)):
            for r in range(R):
                if int(h[i]) not in heads[r] or int(t[i]) not in tails[r]:
                    ok[i, r] = False
    return ok


def reference_scores(con, h, t):
    """kge_predict of (h_i, t_i, r) for every query and relation: one call per relation, so TransR uses r's own matrix."""
    h, t = np.asarray(h), np.asarray(t)
    return np.stack([con.test_step(h, t, np.full(len(h), r)).reshape(-1) for r in range(con.relTotal)], axis=1)


def random_pairs(con, n=48, seed=0):
    rng = np.random.default_rng(seed)
    h = rng.integers(0, con.entTotal, n)
    t = rng.integers(0, con.entTotal, n)
    h[5:9] = h[0]; t[5:9] = t[0]      # duplicates
    t[10] = h[10]                     # h == t
    return h, t


def tol(x):
    return 1e-6 + 1e-5 * np.abs(x)


def assert_row(ids, sc, ref, eligible, k, what):
    """The k best eligible relations of one query against the reference scores: padding, ascending (score, id) order, NaN
    last, scores within an ulp-level tolerance, and no eligible relation with a clearly better score left out."""
    cand = np.nonzero(eligible)[0]
    n_real = min(k, len(cand))
    assert (ids[n_real:] == -1).all() and np.isposinf(sc[n_real:]).all(), what
    ids, sc = ids[:n_real], sc[:n_real]
    assert len(np.unique(ids)) == n_real and eligible[ids].all(), what
    nan = np.isnan(ref)
    want_nan = max(0, n_real - int((~nan[cand]).sum()))
    assert np.isnan(sc).sum() == want_nan and np.isnan(sc[n_real - want_nan:]).all(), what
    fin = ~np.isnan(sc)
    s, i = sc[fin], ids[fin]
    assert (np.abs(s - ref[i]) <= tol(ref[i])).all(), what
    assert ((s[1:] > s[:-1]) | ((s[1:] == s[:-1]) & (i[1:] > i[:-1]))).all(), what
    if fin.any():
        worst = ref[i].max()
        rest = eligible.copy(); rest[ids] = False; rest &= ~nan
        assert (ref[rest] >= worst - tol(worst)).all(), what


CASES = [("TransE", 16), ("TransE", 40), ("TransE", 200), ("TransE", 512),
         ("TransH", 16), ("TransH", 40), ("TransH", 200),
         ("TransD", 16), ("TransD", 40), ("TransD", 200),
         ("TransR", 16), ("TransR", 40), ("TransR", 200)]


@gpu
@pytest.mark.parametrize("model,dim", CASES)
def test_top_k_relations_equal_predict_per_relation(model, dim):
    con = make_config(model, dim)
    R = con.relTotal
    h, t = random_pairs(con)
    ref = reference_scores(con, h, t)
    everything = np.ones(R, bool)
    for k in (1, 7, R, R + 5, 1024):
        ids, sc = con.top_k_relations(h, t, k)
        assert ids.shape == (len(h), k) and ids.dtype == np.int64 and sc.dtype == np.float32
        for i in range(len(h)):
            assert_row(ids[i], sc[i], ref[i], everything, k, (model, dim, k, i))
    # the raw top-R list is the reference's order, up to near-ties
    ids, _ = con.top_k_relations(h, t, R)
    want = np.argsort(ref, axis=1, kind="stable")
    assert (ids == want).mean() > 0.9


@gpu
@pytest.mark.parametrize("model", ["TransE", "TransR"])
def test_filter_and_types_against_dataset_masks(model):
    con = make_config(model, 40)
    R = con.relTotal
    h, t = random_pairs(con, n=40, seed=3)
    th, tt, _ = sorted_test_triples(KG)        # pairs with known relations, so the filter has work to do
    h = np.concatenate([h, th[:40]]); t = np.concatenate([t, tt[:40]])
    ref = reference_scores(con, h, t)
    for filtered, typed in ((True, False), (False, True), (True, True)):
        ok = masks(KG, h, t, R, filtered, typed)
        for k in (3, R):
            ids, sc = con.top_k_relations(h, t, k, filtered=filtered, type_constrained=typed)
            for i in range(len(h)):
                assert_row(ids[i], sc[i], ref[i], ok[i], k, (model, filtered, typed, k, i))
    assert not masks(KG, th[:40], tt[:40], R, True, False).all()   # the filter removed something


def brute_counts(ref, r_true, ok_f, ok_t):
    """[n, 4] raw / filtered / typed / filtered + typed counts of relations r' != r strictly below the true score, and the
    number of relations within tolerance of it (rows where the device may differ by that much)."""
    n, R = ref.shape
    out = np.zeros((n, 4), np.int64)
    near = np.zeros(n, np.int64)
    for i in range(n):
        s0 = ref[i, r_true[i]]
        other = np.arange(R) != r_true[i]
        below = other & (ref[i] < s0)
        out[i] = [below.sum(), (below & ok_f[i]).sum(), (below & ok_t[i]).sum(), (below & ok_f[i] & ok_t[i]).sum()]
        near[i] = (other & (np.abs(ref[i] - s0) <= tol(s0))).sum()
    return out, near


def check_ranks(con, path, what):
    R = con.relTotal
    h, t, r = sorted_test_triples(path)
    got, met = con.relation_prediction()
    assert got.shape == (len(h), 4) and got.dtype == np.int64 and len(met) == 20
    ref = reference_scores(con, h, t)
    ok_f = masks(path, h, t, R, True, False)
    ok_t = masks(path, h, t, R, False, True)
    want, near = brute_counts(ref, r, ok_f, ok_t)
    diff = np.abs(got - want).max(axis=1)
    assert (diff <= near).all(), (what, np.nonzero(diff > near)[0][:5])
    assert (got[:, 1] <= got[:, 0]).all() and (got[:, 3] <= got[:, 2]).all() and (got[:, 2] <= got[:, 0]).all()
    # raw count == position of r in the unfiltered top-R list
    ids, _ = con.top_k_relations(h, t, R)
    pos = np.argmax(ids == r[:, None], axis=1)
    clean = near == 0
    assert np.array_equal(pos[clean], got[clean, 0]), what
    # a part of a range gives the same rows
    part, _ = con.relation_prediction(first=3, count=10)
    assert np.array_equal(part, got[3:13])
    return got


@gpu
@pytest.mark.parametrize("model", ["TransE", "TransH", "TransD", "TransR"])
def test_relation_ranks_against_brute_force(model):
    check_ranks(make_config(model, 40), KG, model)


@gpu
@pytest.mark.parametrize("model", ["TransE", "TransR"])
def test_relation_ranks_on_typed_graph(tmp_path, model):
    from openkeonspark_amd.synthetic import make_typed_dataset, SMALL_TYPED
    path = make_typed_dataset(str(tmp_path / "typed"), SMALL_TYPED)
    got = check_ranks(make_config(model, 32, path=path), path, model)
    assert got[:, 2].sum() < got[:, 0].sum()      # the type lists constrain something


def test_relation_metric_reduction():
    """The 20 rel* metrics of a hand-made [count, 4] array: MR, MRR and Hits@1/3/10 of each column."""
    from openkeonspark_amd import rank_eval
    out = np.array([[0, 0, 0, 0], [3, 1, 0, 0], [12, 9, 2, 1], [2, 2, 1, 1], [30, 0, 9, 0]], np.int64)
    d = rank_eval.normalise(rank_eval.rel_sums(out), len(out))
    assert len(d) == 20
    for col, name, suffix in ((0, "", ""), (1, "_filter", ""), (2, "", "_constrain"), (3, "_filter", "_constrain")):
        c = out[:, col]
        assert d["rel" + name + "_tot" + suffix] == pytest.approx(np.mean(c < 10))
        assert d["rel3" + name + "_tot" + suffix] == pytest.approx(np.mean(c < 3))
        assert d["rel1" + name + "_tot" + suffix] == pytest.approx(np.mean(c < 1))
        assert d["rel" + name + "_rank" + suffix] == pytest.approx(np.mean(c + 1))
        assert d["rel" + name + "_reci_rank" + suffix] == pytest.approx(np.mean(1.0 / (c + 1)))


@gpu
@pytest.mark.parametrize("model", ["TransE", "TransR"])
def test_chunking_is_bit_identical(tmp_path, model):
    from openkeonspark_amd.synthetic import make_typed_dataset, SMALL_TYPED
    path = make_typed_dataset(str(tmp_path / "manyrel"), SMALL_TYPED, relations=3000, seed=121)
    con = make_config(model, 16, path=path)
    R = con.relTotal
    assert R == 3000
    h, t, _ = sorted_test_triples(path)
    L = con.lib
    one = con.relation_prediction()[0], con.top_k_relations(h, t, 10, filtered=True)
    try:
        L.kge_set_option(b"relpred_chunk_bytes", R * 4 * 97)     # 97 queries per chunk; TransR: a few relations per block
        many = con.relation_prediction()[0], con.top_k_relations(h, t, 10, filtered=True)
    finally:
        L.kge_set_option(b"relpred_chunk_bytes", 256 << 20)
    assert np.array_equal(one[0], many[0])
    assert np.array_equal(one[1][0], many[1][0])
    assert np.array_equal(one[1][1].view(np.uint32), many[1][1].view(np.uint32))


@gpu
def test_ties_and_nan():
    import torch
    con = make_config("TransE", 32)
    R = con.relTotal
    rel = con._tables[1]
    with torch.no_grad():
        rel[7].copy_(rel[3])             # identical relation rows: identical scores, the smaller id first
        rel[5].fill_(float("nan"))       # a NaN relation: sorts after every number, never counted
    con.tables_changed()
    h, t = random_pairs(con, n=20, seed=5)
    ids, sc = con.top_k_relations(h, t, R)
    for i in range(len(h)):
        p3, p7 = np.nonzero(ids[i] == 3)[0][0], np.nonzero(ids[i] == 7)[0][0]
        assert p7 == p3 + 1 and sc[i, p3] == sc[i, p7]
        assert ids[i, R - 1] == 5 and np.isnan(sc[i, R - 1]) and not np.isnan(sc[i, :R - 1]).any()
    th, tt, tr = sorted_test_triples(KG)
    got, _ = con.relation_prediction()
    for i in range(len(th)):
        if tr[i] == 5:
            assert (got[i] == 0).all()     # a NaN true score counts nothing
        else:
            assert got[i, 0] <= R - 2      # the NaN relation is never below it
    ref = reference_scores(con, th, tt)
    ok_f = masks(KG, th, tt, R, True, False)
    ok_t = masks(KG, th, tt, R, False, True)
    want, near = brute_counts(ref, tr, ok_f, ok_t)
    assert (np.abs(got - want).max(axis=1) <= near).all()


_TRAIN_SEQUENCE = """
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
import openkeonspark_amd as pkg
con = pkg.Config()
con.set_in_path(%r); con.set_work_threads(1); con.set_dimension(32); con.set_test_link_prediction(True)
con.init()
con.set_model_and_session(pkg.%s)
con.train_step()
if %r:
    con.relation_prediction()
    con.top_k_relations([1, 2, 3], [4, 5, 6], 5, filtered=True)
con.train_step()
torch.cuda.synchronize()
np.savez(%r, **con.get_parameters())
"""


@gpu
@pytest.mark.parametrize("model", ["TransE", "TransR"])
def test_no_interference_with_training(tmp_path, model):
    """train step -> relation prediction -> train step leaves the tables as train step -> train step does.  Each sequence in
    a fresh process (the engine's training state is process-global).  Training itself adds fp32 gradients with atomics, so two
    runs of the same sequence may differ in the last bits: the sequence with relation prediction must stay within that
    run-to-run spread (stale training state would move whole rows)."""
    runs = []
    for i, with_eval in enumerate((True, False, False)):
        path = str(tmp_path / ("%s_%d.npz" % (model, i)))
        code = _TRAIN_SEQUENCE % (ROOT, KG, model, with_eval, path)
        res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        runs.append(np.load(path))
    a, b, b2 = runs
    for k in b.files:
        noise = np.abs(b[k] - b2[k]).max()
        scale = np.abs(b[k]).max()
        assert np.abs(a[k] - b[k]).max() <= max(4 * noise, 1e-6 * scale), (k, np.abs(a[k] - b[k]).max(), noise)
        assert np.abs(a[k] - b[k]).max() <= 1e-4 * scale, k


@gpu
def test_argument_errors():
    from openkeonspark_amd import KgeError
    con = make_config("TransE", 16)
    E = con.entTotal
    for k in (0, 1025):
        with pytest.raises(KgeError):
            con.top_k_relations(1, 2, k)
    for h, t in ((E, 0), (-1, 0), (0, E), (0, -1)):
        with pytest.raises(KgeError):
            con.top_k_relations(h, t, 5)
    con._sharded = lambda name: True   # as on a rank holding a shard of the entity table
    with pytest.raises(KgeError):
        con.top_k_relations(1, 2, 5)
    with pytest.raises(KgeError):
        con.relation_prediction()
    del con._sharded
    ids, _ = con.top_k_relations([1, 2], 3, 5)
    assert ids.shape == (2, 5)


@gpu
def test_missing_evaluation_files_raise(tmp_path):
    """In a process of its own: the evaluation files are library-global once any Config has imported them."""
    untyped = str(tmp_path / "untyped")
    os.makedirs(untyped)
    for name in ("entity2id.txt", "relation2id.txt", "train2id.txt", "valid2id.txt", "test2id.txt"):
        shutil.copy(os.path.join(KG, name), untyped)
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        import openkeonspark_amd as pkg
        from openkeonspark_amd import KgeError
        def make(path, lp):
            con = pkg.Config()
            con.set_in_path(path); con.set_work_threads(1); con.set_dimension(16); con.set_test_link_prediction(lp)
            con.init()
            con.set_model_and_session(pkg.TransE)
            return con
        con = make(%r, False)
        for call in (lambda: con.top_k_relations(1, 2, 5, filtered=True), lambda: con.top_k_relations(1, 2, 5, type_constrained=True),
                     lambda: con.relation_prediction(0, 3)):
            try:
                call()
            except KgeError as e:
                print("raised:", e)
            else:
                raise SystemExit("no error")
        assert con.top_k_relations(1, 2, 5)[0].shape == (1, 5)
        con = make(%r, True)   # test files, no type_constrain.txt
        try:
            con.top_k_relations(1, 2, 5, type_constrained=True)
        except KgeError as e:
            print("raised:", e)
        else:
            raise SystemExit("no error")
        out, met = con.relation_prediction()
        assert (out[:, 2:] == 0).all() and met["rel_rank_constrain"] == 1.0
        print("ok")
    """) % (ROOT, KG, untyped)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count("raised:") == 4 and "importTestFiles" in res.stdout and "importTypeFiles" in res.stdout
    assert res.stdout.rstrip().endswith("ok")


@gpu
def test_device_tensors_in_device_tensors_out():
    import torch
    con = make_config("TransH", 40)
    h, t = random_pairs(con, n=33, seed=9)
    want_ids, want_sc = con.top_k_relations(h, t, 6, filtered=True)
    for dt in (torch.int32, torch.int64):
        hd = torch.as_tensor(h, dtype=dt, device=con.device)
        td = torch.as_tensor(t, dtype=dt, device=con.device)
        ids, sc = con.top_k_relations(hd, td, 6, filtered=True)
        assert ids.is_cuda and sc.is_cuda and ids.dtype == torch.int64 and sc.dtype == torch.float32
        assert np.array_equal(ids.cpu().numpy(), want_ids)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), want_sc.view(np.uint32))
    ids, _ = con.top_k_relations(int(h[0]), torch.as_tensor(t, device=con.device), 6)
    assert ids.shape == (33, 6) and ids.is_cuda


@gpu
def test_test_dict_and_driver(tmp_path):
    import openkeonspark_amd.distribute_training as dt
    con = make_config("TransE", 16)
    base = con.test()
    assert not any(k.startswith("rel") for k in base)
    con.set_test_relation_prediction(True)
    full = con.test()
    rel = {k: v for k, v in full.items() if k.startswith("rel")}
    assert len(rel) == 20 and set(full) == set(base) | set(rel)
    out = str(tmp_path / "drv")
    os.makedirs(out)
    args = dt.parse_args(["--input_path", KG, "--output_path", out, "--embedding_dimension", "16", "--mode", "test",
                          "--test_relation", "1"])
    dt.main_fun(args)
    res = json.load(open(os.path.join(out, "lp_results.json")))
    assert len([k for k in res if k.startswith("rel")]) == 20 and "r_filter_rank" in res
    assert dt.parse_args(["--input_path", KG]).test_relation == 0


def _rel_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(KG)
    con.set_work_threads(2); con.set_dimension(32); con.set_test_relation_prediction(True)
    con.init()
    torch.manual_seed(0)
    con.set_model_and_session(pkg.TransH)
    for t in con._tables:
        t.mul_(3.0)
    if world > 1:
        con.init_distributed()
    met = con.relation_prediction_distributed()
    if world == 1:
        _, ref = con.relation_prediction()
        assert ref.keys() == met.keys()
        for k in ref:
            assert abs(ref[k] - met[k]) <= 1e-12 * max(1.0, abs(ref[k])), k
    json.dump(met, open(os.path.join(out_dir, "rel_w%d_r%d.json" % (world, rank)), "w"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@gpu
def test_relation_prediction_split_over_ranks(tmp_path):
    import torch.multiprocessing as mp
    port = 30500 + os.getpid() % 1000
    mp.start_processes(_rel_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    mp.start_processes(_rel_worker, args=(2, port + 1, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    one = json.load(open(str(tmp_path / "rel_w1_r0.json")))
    for r in (0, 1):
        two = json.load(open(str(tmp_path / ("rel_w2_r%d.json" % r))))
        assert one.keys() == two.keys() and len(one) == 20
        for k in one:
            assert abs(one[k] - two[k]) <= 1e-12 * max(1.0, abs(one[k])), k
    assert one["rel_rank"] >= one["rel_filter_rank"] >= 1.0


@gpu
def test_training_improves_relation_mrr(tmp_path):
    from openkeonspark_amd.synthetic import make_typed_dataset, SMALL_TYPED
    import openkeonspark_amd as pkg
    path = make_typed_dataset(str(tmp_path / "learn"), SMALL_TYPED)
    con = pkg.Config()
    con.set_in_path(path); con.set_work_threads(4); con.set_dimension(32)
    con.set_nbatches(10); con.set_alpha(0.01); con.set_margin(1.0); con.set_ent_neg_rate(1)
    con.set_test_relation_prediction(True)
    con.init()
    con.set_model_and_session(pkg.TransE)
    before = con.relation_prediction()[1]["rel_filter_reci_rank"]
    for _ in range(30 * con.nbatches):
        con.train_step()
    after = con.relation_prediction()[1]["rel_filter_reci_rank"]
    assert after > before, (before, after)
