"""Batched top-k entity prediction (Config.top_k_tails / top_k_heads, kge_topk_entities): ids and scores against the
predict op over all candidates (ids in order, scores within an ulp-level tolerance), the filtered / type-constrained selections against the pinned ranker's counts
and against masks built from the dataset files, the candidate-table path against the on-the-fly path, ties / NaN /
padding order, the cross-slice merge on a large entity table, argument checks and device-tensor inputs."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

KG = os.path.join(GOLDEN, "kg_small")


def make_config(model="TransE", dim=32, link_prediction=True):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.set_in_path(KG)
    con.set_work_threads(1)
    con.set_dimension(dim)
    con.set_test_link_prediction(link_prediction)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    for t in con._tables:      # spread the scores: xavier-initialised tables rank almost at random
        t.mul_(3.0)
    return con


def random_queries(con, n=64, seed=0):
    rng = np.random.default_rng(seed)
    fixed = rng.integers(0, con.entTotal, n)
    rel = rng.integers(0, con.relTotal, n)
    head = rng.integers(0, 2, n).astype(bool)
    fixed[5:9] = fixed[0]; rel[5:9] = rel[0]; head[5:9] = head[0]     # duplicates
    return fixed, rel, head


def reference_scores(con, f, r, head):
    """kge_predict over every candidate of one query (one call per query: TransR's predict op uses one matrix per call)."""
    E = con.entTotal
    ar = np.arange(E)
    if head:
        return con.test_step(ar, np.full(E, f), np.full(E, r)).reshape(-1)
    return con.test_step(np.full(E, f), ar, np.full(E, r)).reshape(-1)


def top_k(con, f, r, head, k, **kw):
    return (con.top_k_heads if head else con.top_k_tails)(f, r, k, **kw)


def close(a, b):
    return np.abs(a - b) <= 1e-6 + 1e-5 * np.abs(b)


def assert_rows_match(got_ids, got_sc, ref, k, what):
    """Against the predict op's scores `ref` over all candidates: the returned ids are the reference's k best up to
    candidates within an ulp-level tolerance of each other (the two kernels contract the score's products differently),
    each returned score is its candidate's reference score within that tolerance, the order is ascending (score, id),
    NaN scores come after every number and the row is padded with -1 / +inf."""
    E = len(ref)
    n_real = min(k, E)
    assert (got_ids[n_real:] == -1).all() and np.isposinf(got_sc[n_real:]).all(), what
    ids, sc = got_ids[:n_real], got_sc[:n_real]
    assert len(np.unique(ids)) == n_real and ids.min() >= 0 and ids.max() < E, what
    nan = np.isnan(ref)
    want_nan = min(n_real, max(0, n_real - int((~nan).sum())))
    assert np.isnan(sc).sum() == want_nan and np.isnan(sc[n_real - want_nan:]).all(), what
    fin = ~np.isnan(sc)
    assert close(sc[fin], ref[ids[fin]]).all(), what
    s, i = sc[fin], ids[fin]
    assert ((s[1:] > s[:-1]) | ((s[1:] == s[:-1]) & (i[1:] > i[:-1]))).all(), what
    if fin.any():
        worst = ref[i].max()
        rest = np.ones(E, bool); rest[ids] = False; rest &= ~nan
        assert (ref[rest] >= worst - (1e-6 + 1e-5 * abs(worst))).all(), what
    want = np.argsort(ref, kind="stable")[:n_real]
    assert (ids == want).mean() > 0.9 or n_real < 10, what


def assert_rows_equal(got_ids, got_sc, want_ids, want_sc, what):
    assert np.array_equal(got_ids, want_ids), what
    assert np.array_equal(got_sc.view(np.uint32), want_sc.view(np.uint32)), what


def run_mixed(con, fixed, rel, head, k, **kw):
    """Both sides in one batch through the C ABI (the Config methods ask one side per call)."""
    import ctypes
    import torch
    from openkeonspark_amd import _lib
    dev = con.device
    f = torch.as_tensor(fixed, dtype=torch.int32, device=dev)
    r = torch.as_tensor(rel, dtype=torch.int32, device=dev)
    h = torch.as_tensor(head.astype(np.int32), device=dev)
    n = len(fixed)
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    sc = torch.empty((n, k), dtype=torch.float32, device=dev)
    _lib.check(con.lib.kge_topk_entities(ctypes.byref(con._desc), con._tab_ptrs, f.data_ptr(), r.data_ptr(), h.data_ptr(), n, k,
                                         kw.get("flags", 0), ids.data_ptr(), sc.data_ptr(), con._stream()), con.lib)
    return ids.cpu().numpy().astype(np.int64), sc.cpu().numpy()


CASES = [("TransE", 16), ("TransE", 30), ("TransE", 40), ("TransE", 100), ("TransE", 200), ("TransE", 512), ("TransE", 520),
         ("TransH", 16), ("TransH", 40), ("TransH", 200),
         ("TransD", 16), ("TransD", 40), ("TransD", 200),
         ("TransR", 16), ("TransR", 40), ("TransR", 200)]


@pytest.mark.parametrize("model,dim", CASES)
def test_topk_equals_predict_over_all_candidates(model, dim):
    con = make_config(model, dim)
    E = con.entTotal
    fixed, rel, head = random_queries(con)
    ref = [reference_scores(con, f, r, h) for f, r, h in zip(fixed, rel, head)]
    for k in (1, 7, 64, E, 1024):
        ids, sc = run_mixed(con, fixed, rel, head, k)
        assert ids.shape == (len(fixed), k) and sc.dtype == np.float32
        for i in range(len(fixed)):
            assert_rows_match(ids[i], sc[i], ref[i], k, (model, dim, k, i))
        # duplicated queries give identical rows
        for i in range(5, 9):
            assert_rows_equal(ids[i], sc[i], ids[0], sc[0], (model, dim, k, i))
    # the Config methods: one side per call, numpy out
    tails = head == 0
    ids, sc = con.top_k_tails(fixed[tails], rel[tails], 7)
    assert ids.dtype == np.int64 and sc.dtype == np.float32
    mixed_ids, mixed_sc = run_mixed(con, fixed, rel, head, 7)
    for row, i in enumerate(np.nonzero(tails)[0]):
        assert_rows_equal(ids[row], sc[row], mixed_ids[i], mixed_sc[i], (model, dim, "tails", i))


def read_types(path, R):
    a = np.array(open(path).read().split(), dtype=np.int64)
    heads, tails = [set() for _ in range(R)], [set() for _ in range(R)]
    p = 1
    for _ in range(R):
        if p + 1 >= len(a):
            break
        rel, tot = a[p], a[p + 1]; p += 2
        heads[rel] = set(a[p:p + tot].tolist()); p += tot
        if p + 1 >= len(a):
            break
        rel, tot = a[p], a[p + 1]; p += 2
        tails[rel] = set(a[p:p + tot].tolist()); p += tot
    return heads, tails


def read_triples(name):
    a = np.loadtxt(os.path.join(KG, name), skiprows=1, dtype=np.int64).reshape(-1, 3)
    return a   # (h, t, r)


@pytest.mark.parametrize("model", ["TransE", "TransH", "TransR"])
def test_filter_and_types_agree_with_the_ranker(model):
    con = make_config(model, 24)
    E, R = con.entTotal, con.relTotal
    test = read_triples("test2id.txt")
    known = np.concatenate([read_triples(n) for n in ("train2id.txt", "valid2id.txt", "test2id.txt")])
    known_set = set(map(tuple, known.tolist()))
    head_types, tail_types = read_types(os.path.join(KG, "type_constrain.txt"), R)
    # importTestFiles orders the test triples by (r, h, t): the ranker's rows follow that order
    test = test[np.lexsort((test[:, 1], test[:, 0], test[:, 2]))]
    out, _ = con.link_prediction(test_head=True)
    # one call per triple: TransR's predict op uses the matrix of a call's first relation for all of its rows
    predict_target = np.array([con.test_step(test[i:i + 1, 0], test[i:i + 1, 1], test[i:i + 1, 2]).reshape(-1)[0] for i in range(len(test))])
    off_by_one = 0
    for flags in range(4):
        for k in (1, 10, 1000):
            kw = dict(filtered=bool(flags & 1), type_constrained=bool(flags & 2))
            for side, head in ((0, False), (1, True)):
                fixed = test[:, 1] if head else test[:, 0]
                ids, sc = top_k(con, fixed, test[:, 2], head, k, **kw)
                all_ids, all_sc = top_k(con, fixed, test[:, 2], head, 1024)      # every candidate: the target's own score
                target = all_sc[np.arange(len(test)), np.argmax(all_ids == (test[:, 0] if head else test[:, 1])[:, None], axis=1)]
                assert close(target, predict_target).all()
                for i, (h, t, r) in enumerate(test.tolist()):
                    q = int((sc[i] < target[i]).sum())
                    want = min(k, int(out[i, side, flags]))
                    if q != want:
                        off_by_one += 1
                        assert abs(q - want) <= 1, (flags, k, side, i, q, want)
                    got = ids[i][ids[i] >= 0]
                    for c in got.tolist():
                        triple = (c, t, r) if head else (h, c, r)
                        if flags & 1:
                            assert triple not in known_set, (flags, k, side, i, c)
                        if flags & 2:
                            assert c in (head_types[r] if head else tail_types[r]), (flags, k, side, i, c)
                    # nothing eligible was left out: the row is padded only when the eligible set is exhausted
                    eligible = np.ones(E, bool)
                    if flags & 1:
                        for c in range(E):
                            if ((c, t, r) if head else (h, c, r)) in known_set:
                                eligible[c] = False
                    if flags & 2:
                        allowed = np.zeros(E, bool)
                        allowed[list(head_types[r] if head else tail_types[r])] = True
                        eligible &= allowed
                    assert len(got) == min(k, int(eligible.sum())), (flags, k, side, i)
    assert off_by_one <= 4, off_by_one


@pytest.mark.parametrize("model", ["TransE", "TransH", "TransD"])
def test_table_path_equals_direct_path(model):
    con = make_config(model, 40)
    fixed, rel, head = random_queries(con, seed=3)
    L = con.lib
    got = []
    for budget in (1 << 30, 0):
        L.kge_set_option(b"topk_table_max_bytes", budget)
        try:
            got.append([run_mixed(con, fixed, rel, head, k) for k in (1, 10, 300)])
        finally:
            L.kge_set_option(b"topk_table_max_bytes", 1 << 30)
    for (ia, sa), (ib, sb) in zip(*got):
        assert np.array_equal(ia, ib)
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))


def test_ties_go_to_the_smaller_id_and_nan_sorts_last():
    import torch
    con = make_config("TransE", 32)
    E = con.entTotal
    ent = con._tables[0]
    with torch.no_grad():
        ent[100:400] = ent[7]            # 301 equal candidates
        ent[600:610] = float("nan")      # NaN scores
    fixed = np.array([3, 7, 42, 999])
    rel = np.array([0, 1, 2, 3])
    for head in (False, True):
        ref = [reference_scores(con, f, r, head) for f, r in zip(fixed, rel)]
        assert all(np.isnan(x[600:610]).all() for x in ref)
        for k in (5, 350, 1024):
            ids, sc = top_k(con, fixed, rel, head, k)
            for i in range(len(fixed)):
                assert_rows_match(ids[i], sc[i], ref[i], k, (head, k, i))
                tied = np.isin(ids[i], np.arange(100, 400)) | (ids[i] == 7)
                pos = np.nonzero(tied)[0]
                assert (np.diff(ids[i][pos]) > 0).all() and (sc[i][pos] == sc[i][pos[0]]).all() if len(pos) else True
            if k == 1024:
                assert np.array_equal(ids[:, E - 10:E], np.tile(np.arange(600, 610), (len(fixed), 1)))
                assert (ids[:, E:] == -1).all() and np.isposinf(sc[:, E:]).all()


def test_many_slices_merge_exactly():
    import torch
    import openkeonspark_amd as pkg
    E, R, D = 3_000_000, 8, 64
    rng = np.random.default_rng(5)
    n_train = 4096
    h, t, r = rng.integers(0, E, n_train), rng.integers(0, E, n_train), rng.integers(0, R, n_train)
    con = pkg.Config()
    con.set_work_threads(1); con.set_dimension(D); con.set_nbatches(1)
    con.init_from_arrays(E, R, h, t, r)
    con.set_model_and_session(pkg.TransE)
    fixed = rng.integers(0, E, 5)
    rel = rng.integers(0, R, 5)
    L = con.lib
    for k, budget in ((100, 1 << 30), (1024, 1 << 30), (100, 0)):
        L.kge_set_option(b"topk_table_max_bytes", budget)
        try:
            for head in (False, True):
                ids, sc = top_k(con, torch.as_tensor(fixed, device=con.device), torch.as_tensor(rel, device=con.device), head, k)
                for i in range(len(fixed)):
                    reference_scores(con, fixed[i], rel[i], head)
                    s = con.trainModel.predict.reshape(-1)
                    vals, order = torch.sort(s, stable=True)
                    got = ids[i].cpu().numpy()
                    assert_rows_match(got, sc[i].cpu().numpy(), s.cpu().numpy(), k, (k, head, i))
                    assert (ids[i][:10] == order[:10]).float().mean() >= 0.8, (k, head, i)
        finally:
            L.kge_set_option(b"topk_table_max_bytes", 1 << 30)


def test_bad_arguments_raise_before_any_launch():
    from openkeonspark_amd import KgeError
    con = make_config("TransE", 16)
    E, R = con.entTotal, con.relTotal
    for k in (0, 1025):
        with pytest.raises(KgeError):
            con.top_k_tails(1, 0, k)
    with pytest.raises(KgeError):
        con.top_k_tails(E, 0, 5)
    with pytest.raises(KgeError):
        con.top_k_heads(-1, 0, 5)
    with pytest.raises(KgeError):
        con.top_k_tails(1, R, 5)
    ids, _ = con.top_k_tails([1, 2], 0, 5)
    assert ids.shape == (2, 5)


def test_filtered_without_evaluation_files_raises():
    """In a process of its own: the evaluation files are library-global once any Config has imported them."""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        import openkeonspark_amd as pkg
        from openkeonspark_amd import KgeError
        con = pkg.Config()
        con.set_in_path(%r); con.set_work_threads(1); con.set_dimension(16)
        con.init()
        con.set_model_and_session(pkg.TransE)
        for kw in (dict(filtered=True), dict(type_constrained=True)):
            try:
                con.top_k_tails(1, 0, 5, **kw)
            except KgeError as e:
                print("raised:", e)
            else:
                raise SystemExit("no error for %%s" %% kw)
        ids, sc = con.top_k_tails(1, 0, 5)
        assert ids.shape == (1, 5)
        print("ok")
    """) % (ROOT, KG)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count("raised:") == 2 and "importTestFiles" in res.stdout and res.stdout.rstrip().endswith("ok")


def test_device_tensors_in_device_tensors_out():
    import torch
    con = make_config("TransH", 40)
    fixed, rel, _ = random_queries(con, n=33, seed=9)
    want_ids, want_sc = con.top_k_heads(fixed, rel, 12, filtered=True)
    for dt in (torch.int32, torch.int64):
        f = torch.as_tensor(fixed, dtype=dt, device=con.device)
        r = torch.as_tensor(rel, dtype=dt, device=con.device)
        ids, sc = con.top_k_heads(f, r, 12, filtered=True)
        assert ids.is_cuda and sc.is_cuda and ids.dtype == torch.int64 and sc.dtype == torch.float32
        assert np.array_equal(ids.cpu().numpy(), want_ids)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), want_sc.view(np.uint32))
    # a scalar broadcast against a device tensor
    ids, _ = con.top_k_heads(int(fixed[0]), torch.as_tensor(rel, device=con.device), 12)
    assert ids.shape == (33, 12) and ids.is_cuda
