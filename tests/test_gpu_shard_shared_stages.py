"""The two exchange stages of the shared-negatives step on a row-sharded entity table (csrc/shard.hip:
kge_shard_requests_shared, kge_shard_remap_shared), called through the C ABI as train_paths.shared_sharded_step calls them and
compared with numpy written from the header (include/kge_mi355.h, "Table-sharded sparse path").  Integer copies: every comparison
is exact.  Outputs sit between sentinel margins (the Guarded buffers of tests/test_gpu_shard_stages.py)."""
import numpy as np
import pytest

from test_gpu_shard_stages import KGE_ERR_BAD_ARG, SENT, Guarded, _dev, _env, _ok

pytestmark = pytest.mark.gpu

ENT = 1003
P = 5


def make_ids(rng, n_pos, N):
    """Positives and candidate lists with ids of -1 and ids >= ENT among both (where there is room)."""
    n_chunks = -(-n_pos // P) + (1 if n_pos else 0)      # (a slice that begins inside a chunk meets one more)
    h, t = rng.integers(0, ENT, n_pos), rng.integers(0, ENT, n_pos)
    cand = rng.integers(0, ENT, n_chunks * N)
    for a in (h, t, cand):
        if len(a) >= 1:
            a[0] = -1
        if len(a) >= 3:
            a[1], a[-1] = ENT, ENT + 12345
    if n_pos >= 5:
        h[2], t[3] = ENT - 1, 0      # the table's last and first row are inside
    return h, t, cand


def requests_reference(h, t, cand):
    req = np.concatenate([h, t, cand]).astype(np.int64)
    return np.where((req >= 0) & (req < ENT), req, -1)


@pytest.mark.parametrize("N", [1, 25])
@pytest.mark.parametrize("n_pos", [0, 1, 5, 5000])
def test_requests_and_remap(n_pos, N):
    torch, _lib, L = _env()
    rng = np.random.default_rng(100 * n_pos + N)
    h, t, cand = make_ids(rng, n_pos, N)
    n_cand, n_req = len(cand), 2 * n_pos + len(cand)
    d_h, d_t, d_c = _dev(np.append(h, 1 << 30)), _dev(np.append(t, 1 << 30)), _dev(np.append(cand, 1 << 30))
    req = Guarded(max(n_req, 1))
    _ok(L.kge_shard_requests_shared(d_h.data_ptr(), d_t.data_ptr(), n_pos, d_c.data_ptr(), n_cand, ENT, req.ptr(), None), _lib)
    got = req.get()
    want = requests_reference(h, t, cand)
    assert np.array_equal(got[:n_req], want)
    assert (got[n_req:] == SENT).all()
    if n_pos >= 5:
        assert (want == -1).sum() >= 7 and want[2] == ENT - 1 and want[n_pos + 3] == 0
    # positions in a fetched-row list: any injective numbering of the live requests will do for the stage; -1 where there is none
    slot_of = np.full(n_req, -1, np.int64)
    live = np.flatnonzero(want >= 0)
    slot_of[live] = rng.permutation(len(live))
    junk = slot_of.copy()
    junk[want < 0] = 777                                   # a negative id gives -1 whatever d_slot_of holds ...
    neg = np.concatenate([h, t, cand]) < 0
    d_slot = _dev(np.append(np.where(neg, junk, slot_of), SENT))
    h2, t2, c2 = Guarded(max(n_pos, 1)), Guarded(max(n_pos, 1)), Guarded(max(n_cand, 1))
    _ok(L.kge_shard_remap_shared(d_h.data_ptr(), d_t.data_ptr(), n_pos, d_c.data_ptr(), n_cand, d_slot.data_ptr(), h2.ptr(), t2.ptr(),
                                 c2.ptr(), None), _lib)
    for out, lo, n in ((h2, 0, n_pos), (t2, n_pos, n_pos), (c2, 2 * n_pos, n_cand)):
        g = out.get()
        assert np.array_equal(g[:n], slot_of[lo:lo + n])   # ... and an id beyond the table the -1 its request got
        assert (g[n:] == SENT).all()


def test_bad_arguments_write_nothing():
    torch, _lib, L = _env()
    z = _dev(np.zeros(16))
    out = Guarded(16)
    assert L.kge_shard_requests_shared(z.data_ptr(), z.data_ptr(), -1, z.data_ptr(), 2, ENT, out.ptr(), None) == KGE_ERR_BAD_ARG
    assert L.kge_shard_requests_shared(z.data_ptr(), z.data_ptr(), 2, z.data_ptr(), 2, ENT, None, None) == KGE_ERR_BAD_ARG
    assert L.kge_shard_requests_shared(z.data_ptr(), z.data_ptr(), 2, z.data_ptr(), 2, -1, out.ptr(), None) == KGE_ERR_BAD_ARG
    assert L.kge_shard_remap_shared(z.data_ptr(), z.data_ptr(), 2, z.data_ptr(), -2, z.data_ptr(), out.ptr(), out.ptr(), out.ptr(), None) == KGE_ERR_BAD_ARG
    assert L.kge_shard_remap_shared(z.data_ptr(), z.data_ptr(), 2, z.data_ptr(), 2, None, out.ptr(), out.ptr(), out.ptr(), None) == KGE_ERR_BAD_ARG
    assert (out.get() == SENT).all()
