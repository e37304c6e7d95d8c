"""kge_shared_order_by_relation alone: the stable order of a batch by relation, the permuted ids, the chunk table and its count
equal train_paths.shared_relation_chunks -- the numpy statement of the definition (include/kge_mi355.h) -- exactly, slot for slot
up to the cap.  The engine has no size branch of its own in this stage (rocPRIM chooses its sort and scan shapes by size; n_pos
from 1 to 4099 crosses its one-block and many-block forms)."""
import numpy as np
import pytest

from openkeonspark_amd.train_paths import shared_chunk_cap, shared_relation_chunks

pytestmark = pytest.mark.gpu

E = 50
N_POS = [1, 11, 257, 4099]
CHUNKS = [1, 2, 64, 127]


def import_graph(R):
    import openkeonspark_amd as ok
    con = ok.Config()
    con.set_work_threads(1)
    n = max(40, R)
    hh = np.arange(n) % E
    con.init_from_arrays(E, R, hh, (hh + 1) % E, np.arange(n) % R)
    return con


def relation_patterns(n_pos, R, P, rng):
    """name -> relation ids of a batch of n_pos."""
    out = {"random": rng.integers(0, R, n_pos), "with_-1_and_rel_total": rng.integers(-1, R + 1, n_pos),
           "one_relation": np.full(n_pos, R - 1), "far_outside": rng.choice([-7, 0, R - 1, R, R + 100, 2 ** 31 - 1], n_pos)}
    if n_pos <= R:
        out["own_relation"] = rng.permutation(R)[:n_pos]
    if n_pos >= 3:
        out["ends_outside"] = np.r_[-1, rng.integers(0, R, n_pos - 2), R]
    if R >= 4 and n_pos >= 2 * P + 2:      # runs of length 1, 0, P and P + 1; the rest in the trailing run
        lens = [1, 0, P, P + 1]
        ids = np.concatenate([np.full(n, k) for k, n in enumerate(lens)] + [np.full(n_pos - 2 * P - 2, -1)])
        out["runs_0_1_P_P+1"] = ids[rng.permutation(n_pos)]
    return out


def order_on_device(L, h, t, r, P, R):
    import torch
    n_pos = len(r)
    cap = shared_chunk_cap(n_pos, P, R)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    dh, dt, dr = dev(h), dev(t), dev(r)
    perm = torch.full((n_pos,), -5, dtype=torch.int32, device="cuda")
    out = torch.full((3, n_pos), -5, dtype=torch.int32, device="cuda")
    chunks = torch.full((cap + 2, 2), -5, dtype=torch.int32, device="cuda")      # (two guard slots past the cap)
    n_chunks = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    rc = L.kge_shared_order_by_relation(dh.data_ptr(), dt.data_ptr(), dr.data_ptr(), n_pos, P, perm.data_ptr(), out[0].data_ptr(),
                                        out[1].data_ptr(), out[2].data_ptr(), chunks.data_ptr(), n_chunks.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return perm.cpu().numpy(), out.cpu().numpy(), chunks.cpu().numpy(), int(n_chunks.item())


@pytest.mark.parametrize("R", [1, 4, 300])
def test_order_and_chunk_table_equal_the_definition(R):
    con = import_graph(R)
    L = con.lib
    rng = np.random.default_rng(100 + R)
    seen = set()
    for n_pos in N_POS:
        h, t = rng.integers(0, E, n_pos), rng.integers(0, E, n_pos)
        for P in CHUNKS:
            for name, r in relation_patterns(n_pos, R, P, rng).items():
                r = r.astype(np.int64)
                want_perm, want_chunks, want_n = shared_relation_chunks(r, P, R)
                perm, ids, chunks, n_chunks = order_on_device(L, h, t, r, P, R)
                where = (name, n_pos, P, R)
                assert np.array_equal(perm, want_perm), where
                assert np.array_equal(ids[0], h[want_perm]) and np.array_equal(ids[1], t[want_perm]), where
                assert np.array_equal(ids[2], r.astype(np.int32)[want_perm]), where      # the ids as given, not the sort key
                cap = len(want_chunks)
                assert n_chunks == want_n <= cap, where
                assert np.array_equal(chunks[:cap], want_chunks), where
                assert (chunks[cap:] == -5).all(), where                                 # nothing is written past the cap
                seen.add(name)
                if name == "own_relation":
                    assert want_n == n_pos
                if name == "runs_0_1_P_P+1":
                    lens = want_chunks[:want_n, 1].tolist()
                    assert lens[:4] == [1, P, P, 1], (where, lens[:6])                   # run of 1 | run of P | run of P + 1 = P and 1
    assert {"random", "with_-1_and_rel_total", "one_relation", "far_outside", "ends_outside"} <= seen
    if R >= 4:
        assert "runs_0_1_P_P+1" in seen
    if R == 300:
        assert "own_relation" in seen


def test_bad_arguments_are_refused():
    import torch
    from openkeonspark_amd import _lib
    con = import_graph(4)
    L = con.lib
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = z.data_ptr()
    for P in (0, 128):
        assert L.kge_shared_order_by_relation(p, p, p, 4, P, p, p, p, p, p, p, None) < 0
        assert "1..127" in _lib.last_error(L)
    assert L.kge_shared_order_by_relation(p, p, None, 4, 2, p, p, p, p, p, p, None) < 0
    # an empty batch: no chunk
    n = torch.full((1,), 9, dtype=torch.int32, device="cuda")
    assert L.kge_shared_order_by_relation(p, p, p, 0, 2, p, p, p, p, p, n.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(n.item()) == 0
