"""Tables, batches and shared-negatives lists on which TransE is EXACT in fp32, and the premises that make the fp64 references
(tests/bf16_ref.py, tests/shared_neg_ref.py) the bit-exact truth for every kernel.  No device, no engine.

A row has s non-zero elements of one magnitude 2^m, so its norm 2^m sqrt(s) is a power of two (s in {1, 4, 16, 64}) and every
normalised element is 0 or +-2^-a, a <= 3.  Every element of e = h^ + r^ - t^ is then a multiple of 1/8 below 4, every score, hinge
and loss sum a multiple of 1/8 far below 2^21, every gradient and SGD result a short dyadic number: fp32 holds all of them, the
order of a sum does not matter, and exact zeros (both operands zero, non-zeros that cancel, a -0.0 operand), hinge ties and
hinges one quantum (1, 1/2 or 1/4 by width, see `quantum`) either side of zero occur in abundance.

Special rows: entity ZERO_POS all +0.0, ZERO_NEG all -0.0, TINY with four elements 2^-24 (sum of squares 2^-46 < 1e-12: clipped),
relation ZERO_REL all +0.0.  The clipped inverse norm 1 / sqrt(1e-12) is 1e6 in fp32 AND in fp64 (asserted), so the zero rows stay
exact wherever they occur.  The TINY row's normalised elements are 15625 * 2^-18: sums with it are still exact in fp32 (asserted),
but a hinge of 2^-18 granularity inside a loss of thousands would make the fp32 loss depend on the order of its sum, so TINY is
scored in every role and never ACTIVE: the batch builder gives its groups negatives the reference found inactive, the list
builder masks the pairs the reference found active.  Its update is tested from hand-made counts (tests/test_gpu_dyadic_rows.py).

`premises` asserts all of this on the references alone; the builders call it before they return, so no device test sees a case
that failed it, and tests/test_dyadic_host.py runs it for every case on a machine without a GPU."""
import functools

import numpy as np

import bf16_ref
import shared_neg_ref

E, R = 500, 7
N_POS, STRIDE = 301, 304
DENOM = 1 << 10
LRS = (1.0, 0.25)
ZERO_POS, ZERO_NEG, TINY, ZERO_REL = 3, 4, 5, 2


def quantum(D):
    """The grid of the hinges at width D.  With q the smallest normalised magnitude, 1 / sqrt(the largest support of a row),
    every |e_j| is a multiple of q and congruent to e_j modulo 2 q, and the elements of a normalised row sum to a multiple of 2 q
    (an even number of equal magnitudes, or the single 1), so every score lies on 2 q Z and every hinge on margin + 2 q Z: 2 q is 1 up to width
    31, 1/2 up to 127, 1/4 from 128 on.  A margin off that grid gives no tie and fails the premises."""
    return 2.0 / np.sqrt(max(s for s in (1, 4, 16, 64) if s <= D // 2))


MARGINS = (0.5, 0.25, 1.0, 0.0)
CLIPPED_INV = 1e6
X_POS, Y_POS = 290, 291            # the groups with exactly 63 (n_neg >= 63) and exactly 64 (n_neg >= 64) active negatives
ROLES = 16                         # the first positives carry the special rows
F32, F64 = np.float32, np.float64


# ---- tables ------------------------------------------------------------------------------------------------------------------

def _dyadic_rows(rng, n, D):
    sizes = [s for s in (1, 4, 16, 64) if s <= D // 2][-2:]
    win = min(D, 24)
    fit = [s for s in sizes if s <= win] or [max(s for s in (1, 4, 16) if s <= win)]      # (64 non-zeros do not fit 24 columns)
    x = np.zeros((n, D), F32)
    for i in range(n):
        where = i % 3                                       # 0: the first `win` columns, 1: the last, 2: anywhere
        s = int(rng.choice(sizes if where == 2 else fit))
        cols = rng.choice(D if where == 2 else win, s, replace=False)
        if where == 1:
            cols = D - 1 - cols
        x[i, cols] = np.ldexp(1.0, int(rng.integers(-2, 2))) * rng.choice([-1.0, 1.0], s)
    x[(x == 0) & (rng.random((n, D)) < 0.5)] = -0.0
    return x


def dyadic_tables(n_ent, n_rel, D, seed):
    """-> (ent [n_ent, D], rel [n_rel, D]) float32, every value a bf16 value."""
    rng = np.random.default_rng(seed)
    ent, rel = _dyadic_rows(rng, n_ent, D), _dyadic_rows(rng, n_rel, D)
    ent[ZERO_POS] = 0.0
    ent[ZERO_NEG] = -0.0
    ent[TINY] = 0.0
    ent[TINY, [0, 1, D - 2, D - 1]] = 2.0 ** -24
    rel[ZERO_REL] = 0.0
    return ent, rel


def normalise(x, f):
    """Rows of x normalised op by op in the float type f, the clamp inside the root as the kernels have it."""
    x = x.astype(f)
    ss = (x * x).sum(-1, keepdims=True, dtype=f)
    clip = f(1e-12)
    return x * (f(1) / np.sqrt(np.where(ss >= clip, ss, clip)))


# ---- one evaluation for batches and lists, in fp32 and fp64 side by side ----------------------------------------------------------

def evaluate(ent, rel, h, t, r, head, row, live, margin):
    """Score positive b against slot k: head[k, b] says whether entity row[k, b] replaces the head (else the tail); live[k, b]
    whether the pair is scored.  Every operation in float32 numpy AND in float64; -> dict(exact: the two agree on every
    normalised row, element of e, score and hinge; v [slots, n_pos] float64; active; zeros: (elements of e over
    scored triples, exact zeros, of which all operands zero, cancelled non-zeros, with a -0.0 operand))."""
    same = lambda a, b: np.array_equal(a.astype(F64), b)
    out = {}
    for f in (F32, F64):
        entn, reln = normalise(ent, f), normalise(rel, f)
        H, T, Rn = entn[h], entn[t], reln[r]
        ep = H + Rn - T
        p = np.abs(ep).sum(1, dtype=f)
        B0, B1 = Rn - T, H + Rn
        v = np.zeros(head.shape, f)
        es = []
        for k in range(head.shape[0]):
            X = entn[np.clip(row[k], 0, len(ent) - 1)]
            e = np.where(head[k][:, None], X + B0, B1 - X)
            v[k] = p - np.abs(e).sum(1, dtype=f) + f(margin)
            es.append(e)
        out[f] = dict(entn=entn, reln=reln, ep=ep, p=p, v=v, es=es)
    a, b = out[F32], out[F64]
    exact = all(same(a[n], b[n]) for n in ("entn", "reln", "ep", "p", "v")) and all(same(x, y) for x, y in zip(a["es"], b["es"]))
    # where the exact zeros come from (fp64 side; raw operands for the sign bit of a zero)
    rh, rt, rr = ent[h], ent[t], rel[r]
    neg0 = lambda x: (x == 0) & np.signbit(x)
    scored = live.any(0)
    total = zeros = both = cancel = minus = 0
    def tally(e, ops, rows_):
        nonlocal total, zeros, both, cancel, minus
        z = (e == 0)[rows_]
        nz = np.zeros_like(z)
        m0 = np.zeros_like(z)
        for o in ops:
            nz |= (o != 0)[rows_]
            m0 |= neg0(o)[rows_]
        total += z.size; zeros += int(z.sum()); both += int((z & ~nz).sum()); cancel += int((z & nz).sum()); minus += int((z & m0).sum())
    tally(b["ep"], (rh, rt, rr), scored)
    for k in range(head.shape[0]):
        x = ent[np.clip(row[k], 0, len(ent) - 1)]
        tally(b["es"][k], (np.where(head[k][:, None], x, rh), np.where(head[k][:, None], rt, x), rr), live[k])
    return dict(exact=exact, v=b["v"], active=live & (b["v"] >= 0), zeros=(total, zeros, both, cancel, minus),
                clipped_inv=(float(F32(1) / np.sqrt(F32(1e-12))), 1.0 / np.sqrt(1e-12)))


def corruption_hinges(entn, reln, h, t, r, margin):
    """For ONE positive: the hinge of every entity as its new tail and as its new head (fp64, exact) -> (v_tail [E], v_head [E],
    e_tail [E, D])."""
    base = entn[h] + reln[r]
    p = np.abs(base - entn[t]).sum()
    e_tail = base[None, :] - entn
    v_tail = p - np.abs(e_tail).sum(1) + margin
    v_head = p - np.abs(entn + (reln[r] - entn[t])[None, :]).sum(1) + margin
    return v_tail, v_head, e_tail


# ---- the sampler-shaped batch -----------------------------------------------------------------------------------------------------

def _role_positives(rng, h, t, r, head, row):
    """The special rows as head, as tail, as relation and as corrupted entity (slot 0) of the first ROLES positives."""
    far = lambda n: 10 + rng.integers(0, E - 10, n)
    h[:ROLES] = far(ROLES)
    t[:ROLES] = 10 + (h[:ROLES] - 10 + 1 + rng.integers(0, E - 11, ROLES)) % (E - 10)
    h[0], t[1], h[2], t[3], h[4], t[5], r[6] = ZERO_POS, ZERO_POS, ZERO_NEG, ZERO_NEG, TINY, TINY, ZERO_REL
    h[7], t[7], r[7] = ZERO_POS, ZERO_NEG, ZERO_REL             # a positive whose e is zero in every element
    for b, (is_head, ident) in zip(range(8, 14), ((True, ZERO_POS), (False, ZERO_POS), (True, ZERO_NEG), (False, ZERO_NEG), (True, TINY),
                                                  (False, TINY))):
        head[0, b], row[0, b] = is_head, ident


def _materialise(h, t, r, head, row):
    n_neg = head.shape[0]
    bh, bt, br = (np.zeros(STRIDE * (1 + n_neg), np.int32) for _ in range(3))
    bh[:N_POS], bt[:N_POS], br[:N_POS] = h, t, r
    for k in range(n_neg):
        s = slice((k + 1) * STRIDE, (k + 1) * STRIDE + N_POS)
        bh[s], bt[s], br[s] = np.where(head[k], row[k], h), np.where(head[k], t, row[k]), r
    return bh, bt, br


def build_batch(D, n_neg, margin, seed=0):
    """Tables and a sampler-shaped batch (layout of tests/test_gpu_bf16_emit.sampler_shaped_batch, entity negatives only) with the
    role positives, sixty slots overwritten with negatives the reference scores at exactly 0, plus and minus one quantum, the TINY groups made
    inactive and, from 63 negatives on, the boundary groups.  Raises AssertionError where the premises fail."""
    ent, rel = dyadic_tables(E, R, D, 7 * D + seed)
    rng = np.random.default_rng(1000 * D + 10 * n_neg + seed)
    h = rng.integers(0, E, N_POS); t = (h + 1 + rng.integers(0, E - 1, N_POS)) % E; r = rng.integers(0, R, N_POS)
    head = rng.integers(0, 2, (n_neg, N_POS)).astype(bool)
    row = rng.integers(0, E, (n_neg, N_POS))
    row[row == TINY] = TINY + 1                                 # TINY only where it is placed on purpose
    h[h == TINY] += 1; t[t == TINY] += 1
    t[h == t] = 10 + (t[h == t] + 7) % (E - 10)
    _role_positives(rng, h, t, r, head, row)
    clash = row == np.where(head, h[None, :], t[None, :])
    row[clash] = 10 + (row[clash] + 7) % (E - 10)
    entn, reln = normalise(ent, F64), normalise(rel, F64)
    ids = np.arange(E)

    def candidates(b):
        v_tail, v_head, e_tail = corruption_hinges(entn, reln, h[b], t[b], r[b], margin)
        ok_t, ok_h = (ids != t[b]) & (ids != TINY), (ids != h[b]) & (ids != TINY)
        return v_tail, v_head, ok_t, ok_h, e_tail

    # hinge ties and one-quantum misses, slot 0 of the positives from ROLES on
    need = {0.0: 20, quantum(D): 20, -quantum(D): 20}
    for b in range(ROLES, X_POS):
        want = next((w for w, n in need.items() if n > 0), None)
        if want is None:
            break
        v_tail, v_head, ok_t, ok_h, _ = candidates(b)
        hit_t, hit_h = np.nonzero(ok_t & (v_tail == want))[0], np.nonzero(ok_h & (v_head == want))[0]
        if len(hit_t) or len(hit_h):
            head[0, b], row[0, b] = (False, hit_t[0]) if len(hit_t) else (True, hit_h[0])
            need[want] -= 1
    # TINY as head or tail of the positive: every negative of the group from the inactive ones;  TINY as the corrupted entity:
    # the positive redrawn until the pair is inactive
    for b in (4, 5):
        v_tail, v_head, ok_t, ok_h, _ = candidates(b)
        off = [(False, c) for c in np.nonzero(ok_t & (v_tail < 0))[0]] + [(True, c) for c in np.nonzero(ok_h & (v_head < 0))[0]]
        assert off, "no inactive negative for a TINY group"
        for k in range(n_neg):
            head[k, b], row[k, b] = off[(k * 37) % len(off)]
    for b in (12, 13):
        for _ in range(600):
            v_tail, v_head, _ = corruption_hinges(entn, reln, h[b], t[b], r[b], margin)
            if (v_head if head[0, b] else v_tail)[TINY] < 0:
                break
            h[b] = 10 + rng.integers(0, E - 10); t[b] = 10 + (h[b] - 10 + 1 + rng.integers(0, E - 11)) % (E - 10); r[b] = rng.integers(0, R)
        clash = row[:, b] == (np.where(head[:, b], h[b], t[b]))
        row[clash, b] = 10 + (row[clash, b] + 7) % (E - 10)
    # exactly 63 and exactly 64 active negatives: the positive is redrawn until it has active and inactive corruptions to choose from
    def redraw(b):
        h[b] = 10 + rng.integers(0, E - 10); t[b] = 10 + (h[b] - 10 + 1 + rng.integers(0, E - 11)) % (E - 10); r[b] = rng.integers(0, R)

    def on_off(b):
        v_tail, v_head, ok_t, ok_h, e_tail = candidates(b)
        on = [(False, c) for c in np.nonzero(ok_t & (v_tail >= 0))[0]] + [(True, c) for c in np.nonzero(ok_h & (v_head >= 0))[0]]
        off = [(False, c) for c in np.nonzero(ok_t & (v_tail < 0))[0]] + [(True, c) for c in np.nonzero(ok_h & (v_head < 0))[0]]
        return on, off, ok_t & (v_tail >= 0), e_tail

    if n_neg >= 63:
        for _ in range(400):
            on, off, on_t, e_tail = on_off(X_POS)
            sp = np.sign(entn[h[X_POS]] + reln[r[X_POS]] - entn[t[X_POS]])
            against = on_t[:, None] & (np.sign(e_tail) == -sp[None, :]) & (sp != 0)[None, :]      # active new tails whose sign opposes the positive's
            pool = np.nonzero(against[:, int(against.sum(0).argmax())])[0]
            if len(pool) and off:
                break
            redraw(X_POS)
        assert len(pool) and off, "no positive with an active new tail that opposes it in some column and an inactive negative"
        for k in range(n_neg):
            head[k, X_POS], row[k, X_POS] = (False, pool[k % len(pool)]) if k < 63 else off[(k - 63) % len(off)]
    if n_neg >= 64:
        for _ in range(400):
            on, off, _, _ = on_off(Y_POS)
            if on and off:
                break
            redraw(Y_POS)
        assert on and off
        for k in range(n_neg):
            head[k, Y_POS], row[k, Y_POS] = on[(k * 11) % len(on)] if k < 64 else off[(k - 64) % len(off)]
    bh, bt, br = _materialise(h, t, r, head, row)
    want = bf16_ref.emit(ent, rel, bh, bt, br, N_POS, n_neg, STRIDE, margin, DENOM)
    c = dict(kind="batch", D=D, n_neg=n_neg, margin=margin, ent=ent, rel=rel, h=h, t=t, r=r, head=head, row=row,
             live=np.ones(head.shape, bool), bh=bh, bt=bt, br=br, want=want)
    premises(c)
    return c


# ---- shared-negatives lists -------------------------------------------------------------------------------------------------------

def build_lists(D, P, N, margin, chunks=None, n_pos=None, seed=0):
    """Tables and lists in the layout of tests/test_gpu_shared_emit.make_lists (chunks None: n_pos = 2 P + 3 in chunks of P by
    position) or tests/test_gpu_shared_emit_chunks.make_lists (chunks: an int32 [cap, 2] table of (first position, length)):
    a repeated candidate, a positive's own head as a new tail, ids outside the table, a positive with every pair masked, random
    masks; the special rows as head, tail, relation and candidate; sixty positives chosen so that candidate 0 of their chunk scores
    at exactly 0, plus and minus one quantum; every pair with TINY that the reference finds active is masked."""
    if chunks is None:
        n_pos = n_pos or 2 * P + 3
        table = np.array([[j * P, min(P, n_pos - j * P)] for j in range(-(-n_pos // P))], np.int32)
    else:
        table = np.asarray(chunks, np.int32)
        n_pos = int(table[:, 1].sum())
    cap = len(table)
    used = [j for j in range(cap) if table[j, 1] > 0]
    chunk_of = np.zeros(n_pos, np.int64)
    for j in used:
        chunk_of[table[j, 0]:table[j, 0] + table[j, 1]] = j
    ent, rel = dyadic_tables(E, R, D, 11 * D + P + seed)
    rng = np.random.default_rng(3000 * D + 10 * P + N + seed)
    h = 10 + rng.integers(0, E - 10, n_pos); t = 10 + (h - 10 + 1 + rng.integers(0, E - 11, n_pos)) % (E - 10); r = rng.integers(0, R, n_pos)
    cand = (10 + rng.integers(0, E - 10, (cap, N))).astype(np.int32)
    pair = rng.integers(0, 2, (n_pos, N)).astype(np.uint8)
    # the special rows: as candidates in the last slots, one per chunk of three or more (N = 1 has no other slot); as positives at the first
    # positions of the first chunk and the last position of three chunks
    big = [j for j in used if table[j, 1] >= 3][:3]
    for j, ident in zip(big, (ZERO_POS, ZERO_NEG, TINY)):
        cand[j, N - 1] = ident
    if N >= 6:
        cand[used[0], N - 2], cand[used[0], N - 3] = ZERO_NEG, TINY
        cand[used[0], 1] = cand[used[0], 0]                                  # a repeated candidate
    first = int(table[used[0], 0])
    rest = [j for j in used if j not in big]                                 # TINY as a positive: under ordinary candidates where N = 1
    spots = [int(table[j, 0]) + int(table[j, 1]) - 1 for j in ((rest[:2] if len(rest) >= 2 else big[:2]) + big[2:])]
    assert len(spots) == 3 and table[used[0], 1] >= 4
    h[first], t[first + 1] = ZERO_POS, ZERO_NEG
    h[spots[0]], t[spots[1]], r[spots[2]] = TINY, TINY, ZERO_REL
    entn, reln = normalise(ent, F64), normalise(rel, F64)

    def hinge(hh, tt, rr, c, is_head):
        p = np.abs(entn[hh] + reln[rr] - entn[tt]).sum(-1)
        e = np.where(is_head[..., None], entn[c] + reln[rr] - entn[tt], entn[hh] + reln[rr] - entn[c])
        return p - np.abs(e).sum(-1) + margin

    # ties and one-quantum misses on candidate 0: the positive is redrawn until its hinge hits the value
    need = {0.0: 20, quantum(D): 20, -quantum(D): 20}
    special = set([first, first + 1, first + 2] + spots)
    reserved = {}                                                               # (chunk, slot) with TINY -> a position kept for it
    for j, k in zip(*np.nonzero(cand == TINY)):
        reserved[(int(j), int(k))] = next(b for b in range(int(table[j, 0]), int(table[j, 0] + table[j, 1])) if b not in special)
        special.add(reserved[(int(j), int(k))])
    for b in range(n_pos):
        want = next((w for w, n in need.items() if n > 0), None)
        if want is None:
            break
        c0 = int(cand[chunk_of[b], 0])
        if b in special or c0 == TINY:
            continue
        hh = 10 + rng.integers(0, E - 10, 600); tt = 10 + (hh - 10 + 1 + rng.integers(0, E - 11, 600)) % (E - 10); rr = rng.integers(0, R, 600)
        v = hinge(hh, tt, rr, np.full(600, c0), np.full(600, bool(pair[b, 0] & 1)))
        hit = np.nonzero(v == want)[0]
        if len(hit):
            h[b], t[b], r[b] = hh[hit[0]], tt[hit[0]], rr[hit[0]]
            special.add(b)
            need[want] -= 1
    masked_positive = next(b for b in range(n_pos - 1, -1, -1) if b not in special)
    pair[masked_positive] |= 2                                                  # a positive with every pair masked
    pair[:, 1:] |= (rng.random((n_pos, N - 1)) < 0.1).astype(np.uint8) << 1
    if N >= 8:
        cand[used[0], 2] = E + 3                                                # ids outside the table
        cand[used[1], 3] = -1
        cand[used[0], 4] = h[first + 2]                                         # a positive's own head as a new tail
        pair[first + 2, 4] = 0
    # TINY is scored and never active: its positives and one positive per TINY candidate are redrawn until a pair is scored and
    # inactive, then every pair with TINY that is still active is masked
    c = cand[chunk_of].astype(np.int64)                                            # [n_pos, N]
    ok = (c >= 0) & (c < E)
    for b, slots in [(spots[0], None), (spots[1], None)] + [(b, [k]) for (j, k), b in reserved.items()]:
        if slots is not None:
            pair[b, slots] &= 1
        for _ in range(600):
            open_ = ok[b] & ((pair[b] & 2) == 0)
            v = hinge(np.full(N, h[b]), np.full(N, t[b]), np.full(N, r[b]), np.where(ok[b], c[b], 0), (pair[b] & 1) == 1)
            if (open_ & (v < 0))[slots if slots is not None else slice(None)].any():
                break
            hh = 10 + rng.integers(0, E - 10); tt = 10 + (hh - 10 + 1 + rng.integers(0, E - 11)) % (E - 10)
            h[b], t[b], r[b] = (h[b] if h[b] == TINY else hh), (t[b] if t[b] == TINY else tt), rng.integers(0, R)
    is_head = (pair & 1) == 1
    v = hinge(h[:, None], t[:, None], r[:, None], np.where(ok, c, 0), is_head)
    tiny_pair = (c == TINY) | (h == TINY)[:, None] | (t == TINY)[:, None]
    pair[tiny_pair & ok & (v >= 0)] |= 2
    h, t, r = h.astype(np.int32), t.astype(np.int32), r.astype(np.int32)
    if chunks is None:
        want = shared_neg_ref.forward(ent, rel, h, t, r, cand[:len(used)], pair, P, margin, DENOM)
    else:
        from test_gpu_shared_emit_chunks import forward_chunks
        want = forward_chunks(ent, rel, h, t, r, cand, pair, table, margin, DENOM)
    live = (((pair & 2) == 0) & ok).T                                              # [N, n_pos]
    out = dict(kind="lists", D=D, P=P, N=N, n_pos=n_pos, margin=margin, ent=ent, rel=rel, h=h, t=t, r=r, cand=cand, pair=pair, table=table,
               by_position=chunks is None, head=is_head.T, row=np.where(ok, c, 0).T, live=live, want=want, masked_positive=masked_positive)
    premises(out)
    return out


# ---- the premises -------------------------------------------------------------------------------------------------------------------

def count_grad_fp32(x, counts, denom):
    """g of listed rows op by op in float32, in the kernels' order (count_grad, csrc/transe_counts.hip): unit * inv, d * x^,
    s - d x^, then the product; d = <x^, s>, 0 where the norm was clipped."""
    x, s = np.asarray(x, F32), np.asarray(counts).astype(F32)
    ss = (x * x).sum(1, keepdims=True, dtype=F32)
    uc = ss >= F32(1e-12)
    inv = F32(1) / np.sqrt(np.where(uc, ss, F32(1e-12)))
    xn = x * inv
    d = np.where(uc, (xn * s).sum(1, keepdims=True, dtype=F32), F32(0))
    unit = F32(1) / F32(denom)
    return ((unit * inv) * (s - d * xn)).astype(F32)


def sgd_reference(x, counts, denom, lr):
    """-> (y float32, g float32, y64, g64): the fp64 rule of tests/bf16_ref.py; an element whose gradient is zero keeps its bits."""
    x = np.asarray(x, F32)
    g64 = bf16_ref.gradient(x, counts, denom)
    y64 = x.astype(F64) - float(F32(lr)) * g64
    y = np.where(g64 == 0, x, y64.astype(F32)).astype(F32)
    return y, g64.astype(F32), y64, g64


def touched(c):
    """(rows increasing, counts [n, D] int64) of the case's reference records."""
    w = c["want"]
    return bf16_ref.row_counts(np.asarray(w["keys"]), np.asarray(w["rec"] if "rec" in w else w["records"]))


def premises(c):
    """Conditions on the references alone (see the module's text); AssertionError names the one that fails."""
    ent, rel, D = c["ent"], c["rel"], c["D"]
    for tab in (ent, rel):
        assert np.array_equal(bf16_ref.widen(bf16_ref.to_bf16(tab)).view(np.uint32), tab.view(np.uint32)), "a table value is no bf16 value"
    assert np.signbit(ent[ZERO_NEG]).all() and not ent[ZERO_NEG].any() and not np.signbit(ent[ZERO_POS]).any() and not ent[ZERO_POS].any()
    assert not rel[ZERO_REL].any() and 0 < (ent[TINY].astype(F64) ** 2).sum() < 1e-13
    assert ((ent == 0) & np.signbit(ent)).any() and ((ent == 0) & ~np.signbit(ent)).any()
    ev = evaluate(ent, rel, c["h"], c["t"], c["r"], c["head"], c["row"], c["live"], c["margin"])
    assert ev["clipped_inv"] == (CLIPPED_INV, CLIPPED_INV), "the clipped inverse norm differs between fp32 and fp64"
    assert ev["exact"], "float32 and float64 evaluations differ"
    v, live, act = ev["v"], c["live"], ev["active"]
    h, t, r, head, row = c["h"], c["t"], c["r"], c["head"], c["row"]
    tiny = ((row == TINY) | (h == TINY)[None, :] | (t == TINY)[None, :]) & live
    assert tiny.any() and not (tiny & act).any(), "TINY must be scored and never active"
    dy = live & ~tiny
    QUANTUM = quantum(D)
    assert (np.round(v[dy] / QUANTUM) * QUANTUM == v[dy]).all(), "a hinge is no multiple of the quantum"
    assert np.abs(v[act]).sum() < 2.0 ** 20, "the loss sum could round in fp32"
    want = c["want"]
    counted = act & (act.sum(0) <= bf16_ref.MAX_ACTIVE)[None, :] if c["kind"] == "batch" else act      # (a deferred group adds nothing)
    loss_sum = float(np.where(counted, v, 0.0).sum())
    assert float(np.where(counted, v, 0.0).astype(F32).sum(dtype=F32)) == loss_sum, "the float32 loss sum differs from fp64"
    assert want["loss"] * DENOM == loss_sum and float(F32(want["loss"])) == want["loss"], "the reference loss is not exact in fp32"
    assert (loss_sum / QUANTUM) == round(loss_sum / QUANTUM)
    ties, above, below = (int((dy & (v == x)).sum()) for x in (0.0, QUANTUM, -QUANTUM))
    assert min(ties, above, below) >= 20, ("ties, one quantum above, one below", ties, above, below)
    total, zeros, both, cancel, minus = ev["zeros"]
    assert zeros >= 0.05 * total and both > 0 and cancel > 0 and minus > 0, ("exact zeros of e", ev["zeros"])
    # the zero rows in every role, scored
    sc = live.any(0)
    for ident in (ZERO_POS, ZERO_NEG):
        assert (sc & (h == ident)).any() or (sc & (t == ident)).any(), ("a zero row is no head or tail", ident)
        assert (live & (row == ident)).any(), ("a zero row is no corrupted entity / candidate", ident)
    assert (sc & (h == ZERO_POS)).any() and (sc & (t == ZERO_NEG)).any() and (sc & (r == ZERO_REL)).any()
    assert (sc & (h == TINY)).any() and (sc & (t == TINY)).any() and (live & (row == TINY)).any()
    recs = np.asarray(want["rec"] if "rec" in want else want["records"])
    assert np.abs(recs).max() <= 127, "a record byte exceeds 127"
    if c["kind"] == "batch":
        assert np.array_equal(act.sum(0) * (want["active"] > 0), want["active"]), "the evaluation and tests/bf16_ref.py disagree"
        if c["n_neg"] >= 63:
            assert want["active"][X_POS] == 63 and np.abs(recs.reshape(3 + c["n_neg"], N_POS, D)[:3, X_POS]).max() == 126
            assert (want["keys"].reshape(-1, N_POS)[:3, X_POS] >= 0).all()
        if c["n_neg"] >= 64:
            assert act[:, Y_POS].sum() == 64 and want["active"][Y_POS] == 0 and (want["keys"].reshape(-1, N_POS)[:, Y_POS] == -1).all()
        assert want["deferred"] == int((act.sum(0) > bf16_ref.MAX_ACTIVE).sum()), "deferred groups"      # (others may exceed 63 by themselves)
    # gradients and SGD results of the touched rows: fp32 op by op == fp64, and both survive the float32 round trip
    rows, counts = touched(c)
    assert len(rows) > 10 and TINY not in rows
    x = np.concatenate([ent, rel])[rows]
    g32 = count_grad_fp32(x, counts, DENOM)
    for lr in LRS:
        y, g, y64, g64 = sgd_reference(x, counts, DENOM, lr)
        assert np.array_equal(g.astype(F64), g64) and np.array_equal(g32.astype(F64), g64), "a gradient is not exact in fp32"
        assert np.array_equal(y64.astype(F32).astype(F64), y64), "an SGD result is not exact in fp32"
        y32 = (x - (F32(lr) * g32)).astype(F32)
        assert np.array_equal(y32.astype(F64), y64), "the float32 SGD rule differs from fp64"
    c["stats"] = dict(ties=ties, above=above, below=below, zeros=ev["zeros"], active=int(act.sum()), pairs=int(live.sum()))


def with_margin(build, *args, **kw):
    """The first of MARGINS whose case meets the premises."""
    failed = []
    for margin in MARGINS:
        try:
            return build(*args, margin=margin, **kw)
        except AssertionError as e:
            failed.append((margin, str(e)[:200]))
    raise AssertionError("no margin gives a case that meets the premises: %r" % (failed,))


@functools.lru_cache(maxsize=None)
def batch_case(D, n_neg):
    return with_margin(build_batch, D, n_neg)


@functools.lru_cache(maxsize=None)
def lists_case(D, P, N):
    return with_margin(build_lists, D, P, N, n_pos=4 * P + 3 if N == 1 else None)


def chunk_table(P):
    """Chunks of length P, 1, P - 1, P, 1, then two empty slots (tests/test_gpu_shared_emit_chunks.table_of's shape)."""
    lens = [P, 1, P - 1, P, 1]
    starts = np.cumsum([0] + lens)
    return np.array([[s, n] for s, n in zip(starts[:-1], lens)] + [[int(starts[-1]), 0]] * 2, np.int32)


@functools.lru_cache(maxsize=None)
def chunks_case(D, P, N):
    return with_margin(build_lists, D, P, N, chunks=chunk_table(P))


# the shapes of the device tests (tests/test_gpu_dyadic_*.py) and of tests/test_dyadic_host.py
FP32_DIMS = [10, 16, 50, 72, 200, 264, 512]
BF16_DIMS = [8, 16, 72, 200, 264, 512, 1024]
SHARED_BF16_DIMS = [8, 72, 200, 264, 512]
NEGS = [1, 25, 63]
BOUNDARY_NEG = 70
# (P, N): P is at most 127, so n_pos = 2 P + 3 is 257 or 131; with ONE candidate per chunk, 4 P + 3 = 259 positives in five chunks, so
# that the two zero rows and TINY are candidates and TINY as a positive still meets an ordinary candidate
SHARED_SHAPES = [(64, 1), (64, 25), (127, 63)]
