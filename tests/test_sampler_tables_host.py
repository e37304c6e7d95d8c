"""The sampler's host-built tables (csrc/kg_index.cpp make_jump_digit_table / build_magic_tables), read back through
kge_index_copy as "jump_digits", "ent_magic" and "rel_magic".  No device needed.

jump_digits: entry [k * 512 + d] = (mul, add) of x -> mul * x + add (mod 2^64) after d * 512^k steps of the 64-bit LCG
(Random.h:16-19), four levels.  ent_magic / rel_magic: [sampler_magic_len] entries, entry len = (2^64 - 1) // (total - len) and
0 where the divisor is not positive; the device takes s mod d as s - ((s * m) >> 64) * d followed by two conditional
subtractions, so that difference has to stay below 3 d for every 64-bit s."""
import numpy as np

from openkeonspark_amd.Config import Config

MASK = (1 << 64) - 1
MUL, ADD = 25214903917, 11
E, R = 1000, 4


def table(L, name, cols=None):
    nbytes = L.kge_index_copy(name.encode(), None, 0)
    assert nbytes >= 0, name
    a = np.zeros(nbytes // 8, np.uint64)
    L.kge_index_copy(name.encode(), a.ctypes.data, nbytes)
    return a.reshape(-1, cols) if cols else a


def graph():
    con = Config()
    h = np.arange(3000) % E
    con.init_from_arrays(E, R, h, (h * 7 + 1) % E, h % R)
    return con


def compose(f, g):
    """g after f, both (mul, add)"""
    return (g[0] * f[0]) & MASK, (g[0] * f[1] + g[1]) & MASK


def power(n):
    """n single steps composed, by squaring"""
    out, sq = (1, 0), (MUL, ADD)
    while n:
        if n & 1:
            out = compose(out, sq)
        sq = compose(sq, sq)
        n >>= 1
    return out


def test_jump_digit_entries_are_that_many_single_steps():
    dig = table(graph().lib, "jump_digits", 2)
    assert dig.shape == (4 * 512, 2)
    # levels 0 and 1 one single step after the other (511 * 512 of them), every level against the composed power
    cur = (1, 0)
    for n in range(512 * 512):
        if n < 512:
            assert (int(dig[n, 0]), int(dig[n, 1])) == cur, n
        if n % 512 == 0:
            assert (int(dig[512 + n // 512, 0]), int(dig[512 + n // 512, 1])) == cur, n
        cur = ((MUL * cur[0]) & MASK, (MUL * cur[1] + ADD) & MASK)
    for k in range(4):
        for d in range(512):
            assert (int(dig[k * 512 + d, 0]), int(dig[k * 512 + d, 1])) == power(d * 512 ** k), (k, d)
    # a count written in its digits lands where the single steps do
    x = 1804289383
    for n in (0, 1, 511, 512, 600, 127 * 2100, (1 << 36) - 1):
        y = x
        for k in range(4):
            m, a = (int(v) for v in dig[k * 512 + ((n >> (9 * k)) & 511)])
            y = (m * y + a) & MASK
        pm, pa = power(n)
        assert y == (pm * x + pa) & MASK, n


def check_magic(tab, total, T):
    rng = np.random.default_rng(total + T)
    assert len(tab) == T
    for ln in range(T):
        d, m = total - ln, int(tab[ln])
        if d <= 0:
            assert m == 0, ln
            continue
        assert m == MASK // d, ln
        for s in [0, d - 1, d, MASK] + [int(v) for v in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]:
            rest = s - ((s * m) >> 64) * d
            assert 0 <= rest < 3 * d and rest % d == s % d, (ln, s)


def test_magic_entries_and_their_remainder_bound():
    con = graph()
    L = con.lib
    try:
        check_magic(table(L, "ent_magic"), E, 2048)          # the default length: entries beyond E - 1 are never used (0)
        check_magic(table(L, "rel_magic"), R, 2048)
        assert L.kge_set_option(b"sampler_magic_len", 8) == 0   # rebuilt for the imported set
        check_magic(table(L, "ent_magic"), E, 8)
        check_magic(table(L, "rel_magic"), R, 8)
        con2 = graph()                                       # and built at the lowered length by an import
        assert len(table(con2.lib, "ent_magic")) == 8
    finally:
        L.kge_set_option(b"sampler_magic_len", 2048)
    assert len(table(L, "ent_magic")) == 2048
