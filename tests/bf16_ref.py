"""numpy restatement of bf16 table storage (include/kge_mi355.h, "bf16 table storage"): the stochastic rounding rule in uint64 /
uint32 arithmetic, the emit stage and the two update rules in fp64 on the widened tables.  The tests compare the device with
these; nothing here reads the device."""
import numpy as np

U = np.uint64
GAMMA = U(0x9E3779B97F4A7C15)


def mix64(z):
    """splitmix64's finaliser (csrc/mix_dev.hpp) on uint64 arrays, mod 2^64."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=U)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def step_key(seed, step):
    with np.errstate(over="ignore"):
        return mix64(U(int(seed) & 0xFFFFFFFFFFFFFFFF) + GAMMA * U(int(step) + 1))


def round_bits(seed, step, key, D, j):
    """rnd of column j of the row `key` (arrays broadcast) -> uint32 in [0, 65536)."""
    with np.errstate(over="ignore"):
        key, j = np.asarray(key, dtype=U), np.asarray(j, dtype=U)
        z = mix64(step_key(seed, step) + GAMMA * (key * U(D // 4) + (j >> U(2)) + U(1)))
        return ((z >> (U(16) * (j & U(3)))) & U(0xFFFF)).astype(np.uint32)


def round_stochastic(y, rnd):
    """fp32 y, rnd in [0, 65536) -> the stored uint16 bits."""
    bits = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32)
    rnd = np.asarray(rnd, dtype=np.uint32)
    special = (bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    with np.errstate(over="ignore"):
        return np.where(special, bits >> np.uint32(16), (bits + rnd) >> np.uint32(16)).astype(np.uint16)


def round_rows(y, keys, seed, step):
    """y [rows, D] fp32 stored under the row keys `keys` [rows] at (seed, step) -> uint16 [rows, D]."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    D = y.shape[1]
    rnd = round_bits(seed, step, np.asarray(keys).reshape(-1, 1), D, np.arange(D).reshape(1, -1))
    return round_stochastic(y, rnd)


def widen(b):
    """stored uint16 bits -> fp32, exactly."""
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def to_bf16(x):
    """fp32 -> bf16 bits, round to nearest-even (finite values)."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    with np.errstate(over="ignore"):
        return ((bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def neighbours(y):
    """The two bf16 values around the fp64 value y (finite, inside the bf16 range), as uint16 bits: (towards zero, away from
    zero); equal when y is a bf16 value."""
    y32 = np.asarray(y, dtype=np.float64)
    mag = np.abs(y32)
    f = mag.astype(np.float32)
    f = np.where(f.astype(np.float64) > mag, np.nextafter(f, np.float32(0)), f).astype(np.float32)      # fp32 at or below |y|
    lo = (f.view(np.uint32) >> np.uint32(16)).astype(np.uint32)
    exact = widen(lo.astype(np.uint16)).astype(np.float64) == mag
    hi = np.where(exact, lo, lo + 1)
    sign = np.where(np.signbit(y32), np.uint32(0x8000), np.uint32(0))
    return (lo | sign).astype(np.uint16), (hi | sign).astype(np.uint16)


# ---- the emit stage in fp64 ------------------------------------------------------------------------------------------------------

def normalise(x):
    return x / np.sqrt(np.maximum((x * x).sum(axis=-1, keepdims=True), 1e-12))


MAX_ACTIVE = 63


def emit(ent, rel, bh, bt, br, n_pos, n_neg, stride, margin, denom):
    """The records, keys and loss of the definition on fp32 (widened) tables, in fp64.  Batch layout of Base.cpp: positive b at
    [b], negative k at [b + (k + 1) stride].  -> dict(keys int32 [(3 + n) n_pos], rec int8 [(3 + n) n_pos, D] (zero where the key
    is -1), loss, deferred (groups that are not sampler-shaped, or have more than 63 active negatives), min_sign, min_kink,
    active (active negatives per group that has records))."""
    ent, rel = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    E, D = ent.shape
    b = np.arange(n_pos)
    h, t, r = bh[b], bt[b], br[b]
    hn, tn, rn = normalise(ent[h]), normalise(ent[t]), normalise(rel[r])
    ep = hn + rn - tn
    p = np.abs(ep).sum(axis=1)
    sp = np.sign(ep)
    min_sign = np.abs(ep).min()
    min_kink = np.inf
    keys = np.full((3 + n_neg, n_pos), -1, np.int64)
    rec = np.zeros((3 + n_neg, n_pos, D), np.int64)
    Ah, At, Ar = (np.zeros((n_pos, D), np.int64) for _ in range(3))
    cnt = np.zeros(n_pos, np.int64)
    fast_all = np.ones(n_pos, bool)
    codes, rows = [], []
    for k in range(n_neg):
        j = b + (k + 1) * stride
        nh, nt, nr = bh[j], bt[j], br[j]
        dh, dt, dr = nh != h, nt != t, nr != r
        fast_all &= (dh.astype(int) + dt.astype(int) + dr.astype(int)) == 1
        codes.append(np.where(dh, 0, np.where(dt, 1, 2)))
        rows.append(np.where(dh, nh, np.where(dt, nt, nr)))
    loss = np.zeros(n_pos)
    for k in range(n_neg):
        code, row = codes[k], rows[k]
        xn = np.where((code == 2)[:, None], normalise(rel[np.minimum(row, rel.shape[0] - 1)]), normalise(ent[np.minimum(row, E - 1)]))
        e = np.where((code == 0)[:, None], xn + rn - tn, np.where((code == 1)[:, None], hn + rn - xn, hn + xn - tn))
        v = p - np.abs(e).sum(axis=1) + margin
        s = np.sign(e).astype(np.int64)
        min_sign = min(min_sign, np.abs(e[fast_all]).min() if fast_all.any() else np.inf)
        min_kink = min(min_kink, np.abs(v[fast_all]).min() if fast_all.any() else np.inf)
        act = (v >= 0) & fast_all
        loss += np.where(act, v, 0.0)
        cnt += act
        sa = s * act[:, None]
        c0, c1, c2 = ((code == c)[:, None] for c in range(3))
        rec[3 + k] = np.where(c1, sa, -sa)
        Ah += np.where(c0, 0, -sa); At += np.where(c1, 0, sa); Ar += np.where(c2, 0, -sa)
        keys[3 + k] = np.where(act, np.where(code == 2, E + row, row), -1)
    over = cnt > MAX_ACTIVE      # a positive's int8 sums hold 2 x 63 signs: such a group is deferred like one that is not sampler-shaped
    keys[:, over] = -1
    rec[:, over] = 0
    loss, cnt = np.where(over, 0.0, loss).sum(), np.where(over, 0, cnt)
    live = cnt > 0
    spc = sp.astype(np.int64) * cnt[:, None]
    rec[0] = (Ah + spc) * live[:, None]; rec[1] = (At - spc) * live[:, None]; rec[2] = (Ar + spc) * live[:, None]
    keys[0] = np.where(live, h, -1); keys[1] = np.where(live, t, -1); keys[2] = np.where(live, E + r, -1)
    assert np.abs(rec).max() <= 127
    return dict(keys=keys.reshape(-1).astype(np.int32), rec=rec.reshape(-1, D).astype(np.int8), loss=loss / denom,
                deferred=int((~fast_all).sum() + over.sum()), min_sign=float(min_sign), min_kink=float(min_kink), active=cnt)


def row_counts(keys, rec):
    """Per-row sums of the live records: (sorted rows, counts [n, D] int64)."""
    live = keys >= 0
    rows, inv = np.unique(keys[live], return_inverse=True)
    out = np.zeros((len(rows), rec.shape[1]), np.int64)
    np.add.at(out, inv, rec[live].astype(np.int64))
    return rows, out


# ---- the update rules in fp64 ----------------------------------------------------------------------------------------------------

def gradient(x, counts, denom):
    """g of a listed row from its counts: unit * inv * (s - d x^), d = <x^, s> (0 where the norm was clipped)."""
    x, s = np.asarray(x, np.float64), np.asarray(counts, np.float64)
    ss = (x * x).sum(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(np.maximum(ss, 1e-12))
    xn = x * inv
    d = np.where(ss >= 1e-12, (xn * s).sum(axis=1, keepdims=True), 0.0)
    return (1.0 / denom) * inv * (s - d * xn)


def update(x, counts, denom, lr, acc=None):
    """y (fp64) of the listed rows x (fp32, widened) and, for row-wise Adagrad (acc: [n] fp32), the new accumulators."""
    g = gradient(x, counts, denom)
    lr = float(np.float32(lr))
    if acc is None:
        return np.asarray(x, np.float64) - lr * g, None, g
    a1 = np.asarray(acc, np.float64) + (g * g).sum(axis=1) / g.shape[1]
    return np.asarray(x, np.float64) - lr * g / np.sqrt(a1)[:, None], a1, g
