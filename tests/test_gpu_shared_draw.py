"""kge_shared_negatives_draw: the candidate ids and the side bits against a numpy uint64 restatement of the hashes
(tests/shared_neg_ref.py), the mask bit against set membership in the training triples, and Config.shared_negatives_of."""
import ctypes

import numpy as np
import pytest

import shared_neg_ref as ref

pytestmark = pytest.mark.gpu


def make_graph(E, seed):
    """A few hundred training triples over E entities and 5 relations.  Every entity (up to 64 of them) is a known tail of
    (0, r=0) and a known head of (t=min(3, E-1), r=0): the positive (0, min(3, E-1), 0) is masked whatever is drawn."""
    rng = np.random.default_rng(seed)
    R = 5
    n = 300
    h = rng.integers(0, E, n); t = rng.integers(0, E, n); r = rng.integers(0, R, n)
    full = np.arange(min(E, 64))
    t3 = min(3, E - 1)
    h = np.concatenate([h, np.zeros_like(full), full]); t = np.concatenate([t, full, np.full_like(full, t3)])
    r = np.concatenate([r, np.zeros_like(full), np.zeros_like(full)])
    return R, h.astype(np.int64), t.astype(np.int64), r.astype(np.int64)


@pytest.fixture
def lib():
    from openkeonspark_amd import _lib
    L = _lib.lib()
    yield L
    L.setBern(0)


def import_graph(L, E, R, h, t, r, bern):
    from openkeonspark_amd import _lib
    L.kge_clear_error()
    L.setBern(bern)
    L.setWorkThreads(1)
    L.randReset()
    _lib.check(L.kge_import_train_arrays(E, R, len(h), h.ctypes.data, t.ctypes.data, r.ctypes.data, 0), L)
    prob = np.zeros(R, dtype=np.float32)
    assert L.kge_index_copy(b"bern_prob", prob.ctypes.data, prob.nbytes) == prob.nbytes
    return prob


def draw(L, h, t, r, first_position, P, N, seed, step):
    import torch
    from openkeonspark_amd import _lib
    n_pos = len(h)
    n_chunks = -(-n_pos // P)
    ids = [torch.from_numpy(np.asarray(x, dtype=np.int32)).cuda() for x in (h, t, r)]
    cand = torch.full((n_chunks, N), -5, dtype=torch.int32, device="cuda")
    pair = torch.full((n_pos, N), 0xFF, dtype=torch.uint8, device="cuda")
    _lib.check(L.kge_shared_negatives_draw(ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), n_pos, first_position, P, N, seed,
                                           step, cand.data_ptr(), pair.data_ptr(), None), L)
    torch.cuda.synchronize()
    return cand.cpu().numpy(), pair.cpu().numpy()


def expected(train, E, h, t, r, first_position, P, N, seed, step, prob):
    n_pos = len(h)
    n_chunks = -(-n_pos // P)
    cand = ref.candidates(seed, step, n_chunks, N, E, first_chunk=first_position // P)
    side = ref.sides(ref.side_draws(seed, step, n_pos, N, first_position), r, prob)
    known = set(zip(*train))
    pair = side.copy()
    for b in range(n_pos):
        for k in range(N):
            c = int(cand[b // P, k])
            triple = (int(h[b]), c, int(r[b])) if side[b, k] == 0 else (c, int(t[b]), int(r[b]))
            if triple in known:
                pair[b, k] |= 2
    return cand, pair


@pytest.mark.parametrize("bern", [0, 1])
@pytest.mark.parametrize("step", [0, 12345])
@pytest.mark.parametrize("E", [1, 7, (1 << 20) + 3])
def test_candidates_sides_and_mask(lib, E, step, bern):
    R, th, tt, tr = make_graph(E, E % 1000 + 1)
    prob = import_graph(lib, E, R, th, tt, tr, bern)
    rng = np.random.default_rng(step + 3)
    P, N = 5, 63
    n_pos = 2 * P + 3
    pick = rng.integers(0, len(th), n_pos)
    h, t, r = th[pick].copy(), tt[pick].copy(), tr[pick].copy()
    h[0], t[0], r[0] = 0, min(3, E - 1), 0                      # masked throughout
    h[1], t[1], r[1] = E - 1, 0, 4                              # (very likely) no such group: nothing masked on a side without one
    seed = 0xDEADBEEFCAFEF00D
    for first in (0, 3 * P):
        cand, pair = draw(lib, h, t, r, first, P, N, seed, step)
        want_cand, want_pair = expected((th, tt, tr), E, h, t, r, first, P, N, seed, step, prob if bern else None)
        assert np.array_equal(cand, want_cand)
        assert np.array_equal(pair & 1, want_pair & 1)
        assert np.array_equal(pair, want_pair)
        assert cand.min() >= 0 and cand.max() < E
        if E <= 64:
            assert (pair[0] & 2).all()                          # every entity is a known tail of (0, 0) and a known head of (t3, 0)
    if bern and E == 7:
        assert len(np.unique(prob)) > 1                          # the Bernoulli thresholds differ by relation on this graph
    if E == 7:
        assert {0, 1} <= set(np.unique(pair & 1))


def test_largest_shape_and_bad_arguments(lib):
    """P = 127, N = 63 on more than one workgroup of pairs; the limits are refused with a message."""
    from openkeonspark_amd import _lib
    E = 7
    R, th, tt, tr = make_graph(E, 4)
    import_graph(lib, E, R, th, tt, tr, 0)
    P, N, n_pos = 127, 63, 2 * 127 + 3
    pick = np.arange(n_pos) % len(th)
    h, t, r = th[pick], tt[pick], tr[pick]
    cand, pair = draw(lib, h, t, r, 0, P, N, 1, 2)
    want_cand, want_pair = expected((th, tt, tr), E, h, t, r, 0, P, N, 1, 2, None)
    assert np.array_equal(cand, want_cand) and np.array_equal(pair, want_pair)
    for P_, N_, first, word in ((128, 2, 0, "127"), (2, 64, 0, "63"), (4, 2, 3, "multiple")):
        with pytest.raises(_lib.KgeError, match=word):
            draw(lib, h[:4], t[:4], r[:4], first, P_, N_, 0, 0)


def test_shared_negatives_of_returns_the_step_lists():
    """Through Config: the lists of the step just trained are the hashes of (seed, its global_step) over its positives."""
    import openkeonspark_amd as ok
    E = 200
    R, th, tt, tr = make_graph(E, 11)
    con = ok.Config()
    con.set_work_threads(2); con.set_bern(1); con.set_dimension(32); con.set_ent_neg_rate(6); con.set_rel_neg_rate(0)
    con.set_alpha(0.01); con.set_opt_method("SGD"); con.set_nbatches(4)
    con.set_shared_negatives(16, seed=77)
    con.init_from_arrays(E, R, th, tt, tr)
    con.set_model_and_session(ok.TransE)
    prob = np.zeros(R, dtype=np.float32)
    con.lib.kge_index_copy(b"bern_prob", prob.ctypes.data, prob.nbytes)
    for step in range(2):
        assert con.global_step == step
        con.train_step()
        cand, pair = con.shared_negatives_of(step)
        pos = con._sparse_buf["shared_batch"].cpu().numpy()[:, :con.batch_size]
        assert set(zip(pos[0], pos[1], pos[2])) <= set(zip(th, tt, tr))
        want_cand, want_pair = expected((th, tt, tr), E, pos[0], pos[1], pos[2], 0, 16, 6, 77, step, prob)
        assert cand.shape == (-(-con.batch_size // 16), 6) and pair.shape == (con.batch_size, 6)
        assert np.array_equal(cand, want_cand) and np.array_equal(pair, want_pair)
    with pytest.raises(ok.KgeError):
        con.shared_negatives_of(0)
    con.lib.setBern(0)
