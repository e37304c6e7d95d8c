"""Shared by the type-constrained sampler tests (not a test file): a plain Python / numpy restatement of the whole batch
draw, untyped (Base.cpp:74-143, Corrupt.h:7-101) and typed (include/kge_mi355.h kge_set_typed_sampling), the typed index as
numpy builds it, and a crafted dataset that holds every edge case of the typed draw."""
import os

import numpy as np

MASK = (1 << 64) - 1
GRID_SHAPE = [(7, 1, 0), (64, 2, 1), (64, 25, 0), (50, 3, 0)]    # the committed fixtures' (B, negRate, negRelRate) grid
WIDE_SHAPE = (5, 70, 0)                                            # more than 63 negatives: the one-thread-per-slot kernel
CALLS = 3


def lcg(s):
    return (s * 25214903917 + 11) & MASK       # Random.h:16-19


def thread_slice(B, W, i):
    """Base.cpp:85-92: half-open slice of batch positions owned by virtual thread i."""
    if B % W == 0:
        return i * (B // W), (i + 1) * (B // W)
    per = B // W + 1
    return min(i * per, B), min((i + 1) * per, B)


def _read_longs(path):
    with open(path) as f:
        return [int(x) for x in f.read().split()]


class KG(object):
    """A dataset directory as the sampler sees it: file-order triples, the three filter groups, the Bernoulli table and the
    relation type lists (each sorted, duplicates removed; a relation the file does not name has empty lists)."""

    def __init__(self, path):
        self.path = path
        with open(os.path.join(path, "entity2id.txt")) as f:       # the first number is the total (Reader.h:35-54)
            self.E = int(f.readline().split()[0])
        with open(os.path.join(path, "relation2id.txt")) as f:
            self.R = int(f.readline().split()[0])
        a = _read_longs(os.path.join(path, "train2id.txt"))
        self.train = [(a[1 + 3 * i], a[2 + 3 * i], a[3 + 3 * i]) for i in range(a[0])]     # (h, t, r), file order
        nb = os.path.join(path, "batch2id.txt")
        self.new_batch = _read_longs(nb)[0] if os.path.exists(nb) else 0
        uniq = sorted(set(self.train))
        self.uniq = set(uniq)
        self.tails, self.heads, self.rels = {}, {}, {}
        for h, t, r in uniq:
            self.tails.setdefault((h, r), []).append(t)
            self.heads.setdefault((t, r), []).append(h)
            self.rels.setdefault((h, t), []).append(r)
        for d in (self.tails, self.heads, self.rels):
            for k in d:
                d[k].sort()
        # Reader.h:160-177 and Base.cpp:117 in float, as written there
        freq = np.zeros(self.R, np.float32)
        gl = np.zeros(self.R, np.float32)
        gr = np.zeros(self.R, np.float32)
        for h, t, r in uniq:
            freq[r] += 1
        for (h, r) in self.tails:
            gl[r] += 1
        for (t, r) in self.heads:
            gr[r] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            lm, rm = freq / gl, freq / gr
            self.bern_prob = (np.float32(1000) * rm) / (rm + lm)
        # type lists
        self.raw_head = [[] for _ in range(self.R)]       # as the file has them (repeats kept)
        self.raw_tail = [[] for _ in range(self.R)]
        self.named = set()
        a = _read_longs(os.path.join(path, "type_constrain.txt"))
        p = 1
        while p + 1 < len(a):
            for side in (self.raw_head, self.raw_tail):       # a relation's head line, then its tail line (Reader.h:344-362)
                rel, tot = a[p], a[p + 1]
                side[rel] = a[p + 2:p + 2 + tot]
                self.named.add(rel)
                p += 2 + tot
        self.head_list = [sorted(set(x)) for x in self.raw_head]
        self.tail_list = [sorted(set(x)) for x in self.raw_tail]


def nth_outside(known, n_total, tmp):
    """The tmp-th id (0-based) of range(n_total) that is not in the increasing list `known`: Corrupt.h:25-36 in the closed form
    tmp + #{j : known[j] - j <= tmp}, checked against the enumeration."""
    got = tmp + sum(1 for j, v in enumerate(known) if v - j <= tmp)
    if n_total - len(known) > 0:
        assert got == [x for x in range(n_total) if x not in set(known)][tmp]
    return got


def typed_pick(L, known, s):
    """The typed pick of the specification: None when c = 0 (the caller makes the untyped draw from the same s)."""
    where = {v: i for i, v in enumerate(L)}
    kp = [where[v] for v in known if v in where]           # K': increasing, because both lists are
    c = len(L) - len(kp)
    if c <= 0:
        return None
    tmp = s % c
    pos = tmp + sum(1 for j, v in enumerate(kp) if v - j <= tmp)
    assert L[pos] == [x for x in L if x not in set(known)][tmp]
    return L[pos]


def sample_batch(kg, states, B, neg, negrel, bern, typed):
    """One `sampling` call: returns (h, t, r) int64 arrays in the output layout b + k*B and advances `states` (a list of
    W Python ints) in place.  Also returns, per entity negative, which side was corrupted and whether the typed pick applied:
    info[(b, k)] = (new_tail, c > 0)."""
    W = len(states)
    tot = B * (1 + neg + negrel)
    oh, ot, orr = (np.zeros(tot, np.int64) for _ in range(3))
    info = {}
    n = len(kg.train)
    for i in range(W):
        lef, rig = thread_slice(B, W, i)
        s = states[i]
        for b in range(lef, rig):
            s = lcg(s)                                              # Base.cpp:101-106
            pick = s % kg.new_batch + n - kg.new_batch if kg.new_batch > 0 else s % n
            h, t, r = kg.train[pick]
            oh[b], ot[b], orr[b] = h, t, r
            for k in range(1, neg + 1):
                s = lcg(s)
                prob = kg.bern_prob[r] if bern else np.float32(500)
                new_tail = bool(np.float32(s % 1000) < prob)       # Base.cpp:118, compared in float
                s = lcg(s)
                nh, nt = h, t
                if new_tail:
                    known = kg.tails[(h, r)]
                    v = typed_pick(kg.tail_list[r], known, s) if typed else None
                    nt = v if v is not None else nth_outside(known, kg.E, s % (kg.E - len(known)))
                else:
                    known = kg.heads[(t, r)]
                    v = typed_pick(kg.head_list[r], known, s) if typed else None
                    nh = v if v is not None else nth_outside(known, kg.E, s % (kg.E - len(known)))
                info[(b, k)] = (new_tail, v is not None)
                oh[b + k * B], ot[b + k * B], orr[b + k * B] = nh, nt, r
            for k in range(neg + 1, neg + negrel + 1):              # Base.cpp:133-139
                s = lcg(s)
                known = kg.rels[(h, t)]
                oh[b + k * B], ot[b + k * B] = h, t
                orr[b + k * B] = nth_outside(known, kg.R, s % (kg.R - len(known)))
        states[i] = s
    return oh, ot, orr, info


def typed_index(kg):
    """The typed index as kge_index_copy names it, built with numpy from the definition."""
    i32 = np.int32
    type_tails, type_heads, bounds = [], [], np.zeros((kg.R, 4), i32)
    for r in range(kg.R):
        tl, hl = np.unique(np.array(kg.raw_tail[r], i32)), np.unique(np.array(kg.raw_head[r], i32))
        bounds[r] = (len(type_tails), len(tl), len(type_heads), len(hl))
        type_tails += tl.tolist()
        type_heads += hl.tolist()
    uniq = sorted(kg.uniq)
    U = len(uniq)

    def side(order_key, group_key, member, lists):
        pos = np.full(U, -1, i32)
        count, off = {}, 0
        rows = sorted(uniq, key=order_key)
        while off < U:
            g = group_key(rows[off])
            end = off
            while end < U and group_key(rows[end]) == g:
                end += 1
            L = lists[g[1]]
            found = [L.index(member(x)) for x in rows[off:end] if member(x) in L]
            pos[off:off + len(found)] = found
            count[g] = len(found)
            off = end
        return pos, count

    pos_hr, cnt_hr = side(lambda x: (x[0], x[2], x[1]), lambda x: (x[0], x[2]), lambda x: x[1], kg.tail_list)
    pos_tr, cnt_tr = side(lambda x: (x[1], x[2], x[0]), lambda x: (x[1], x[2]), lambda x: x[0], kg.head_list)
    typed_len = np.array([(cnt_hr[(h, r)], cnt_tr[(t, r)]) for h, t, r in kg.train], i32).reshape(-1, 2)
    return dict(type_tails=np.array(type_tails, i32), type_heads=np.array(type_heads, i32), type_bounds=bounds,
                typed_pos_hr=pos_hr, typed_pos_tr=pos_tr, typed_len=typed_len)


# ---------------------------------------------------------------------------------------------------------------------
# the crafted dataset: E = 12, R = 5
# ---------------------------------------------------------------------------------------------------------------------
CRAFTED_E, CRAFTED_R = 12, 5
CRAFTED_TYPES = {      # relation: (head list, tail list) as written to the file; relation 4 is not named in the file at all
    0: ([0, 4, 5, 9], [1, 2, 3]),
    1: ([0, 1, 1, 2, 7], [5, 5, 6, 8, 8, 9, 10]),            # (c) repeated ids
    2: ([], []),                                             # (d) both counts 0
    3: (list(range(12))[::-1], list(range(12))),             # (f) every entity, the head line unsorted
}


def crafted_triples():
    t = []
    t += [(0, 1, 0), (0, 2, 0), (0, 3, 0)]                   # (a) tails(0, r0) == the tail list of r0: c = 0
    t += [(4, 7, 0), (4, 2, 0)]                              # (b) tail 7 is not in r0's tail list
    t += [(5, 1, 0), (9, 3, 0), (6, 2, 0)]                   # head 6 is not in r0's head list
    t += [(0, 5, 1), (1, 5, 1), (1, 6, 1), (2, 8, 1), (2, 9, 1), (2, 10, 1), (7, 11, 1)]
    t += [(3, 4, 2), (4, 5, 2), (3, 6, 2), (8, 4, 2)]        # r2 has empty lists: always the untyped draw
    t += [(0, x, 3) for x in (1, 2, 3, 4, 5, 6)]             # (e) six known tails inside the list: the binary search
    t += [(1, 2, 3), (2, 3, 3), (2, 4, 3), (1, 4, 3), (3, 4, 3), (3, 5, 3), (3, 6, 3), (4, 5, 3), (4, 6, 3), (4, 7, 3), (4, 8, 3)]   # 1..4
    t += [(x, 11, 3) for x in (5, 6, 7, 8, 9)]               # five known heads of (11, r3)
    t += [(10, 0, 4), (11, 1, 4), (10, 2, 4)]                # r4: no lists in the file
    t += [(0, 1, 0), (2, 9, 1), (4, 5, 3), (4, 5, 3)]        # (g) duplicate lines
    return t


def write_crafted(path):
    """Writes the crafted dataset directory and returns it loaded; asserts that it still holds every case it was made for."""
    os.makedirs(path, exist_ok=True)
    trip = crafted_triples()
    with open(os.path.join(path, "entity2id.txt"), "w") as f:
        f.write("%d\n" % CRAFTED_E)
    with open(os.path.join(path, "relation2id.txt"), "w") as f:
        f.write("%d\n" % CRAFTED_R)
    with open(os.path.join(path, "train2id.txt"), "w") as f:
        f.write("%d\n" % len(trip))
        for h, t, r in trip:
            f.write("%d %d %d\n" % (h, t, r))
    with open(os.path.join(path, "type_constrain.txt"), "w") as f:
        f.write("%d\n" % len(CRAFTED_TYPES))
        for r, (heads, tails) in sorted(CRAFTED_TYPES.items()):
            f.write("%d\t%d%s\n" % (r, len(heads), "".join("\t%d" % x for x in heads)))
            f.write("%d\t%d%s\n" % (r, len(tails), "".join("\t%d" % x for x in tails)))
    kg = KG(path)
    assert_crafted_cases(kg)
    return kg


def assert_crafted_cases(kg):
    assert (kg.E, kg.R) == (CRAFTED_E, CRAFTED_R)
    inside = {g: [v for v in known if v in kg.tail_list[g[1]]] for g, known in kg.tails.items()}
    inside_h = {g: [v for v in known if v in kg.head_list[g[1]]] for g, known in kg.heads.items()}
    # (a) a group whose known tails are exactly the list
    assert any(kg.tail_list[r] and known == kg.tail_list[r] for (h, r), known in kg.tails.items())
    # (b) a known tail outside a non-empty list (and a known head likewise)
    assert any(kg.tail_list[r] and len(inside[(h, r)]) < len(known) for (h, r), known in kg.tails.items())
    assert any(kg.head_list[r] and len(inside_h[(t, r)]) < len(known) for (t, r), known in kg.heads.items())
    # (c) repeated ids in a list
    assert any(len(raw) != len(set(raw)) for raw in kg.raw_tail) and any(len(raw) != len(set(raw)) for raw in kg.raw_head)
    # (d) a relation named with both counts 0 that has training triples; and one the file does not name
    assert any(r in kg.named and not kg.head_list[r] and not kg.tail_list[r] and any(x[2] == r for x in kg.train) for r in range(kg.R))
    assert any(r not in kg.named and any(x[2] == r for x in kg.train) for r in range(kg.R))
    # (e) groups with 1, 2, 3, 4 and more than four known ids inside the list, with candidates left
    for d, lists in ((inside, kg.tail_list), (inside_h, kg.head_list)):
        sizes = {len(v) for g, v in d.items() if len(lists[g[1]]) > len(v)}
        assert {1, 2, 3, 4} <= sizes and max(sizes) > 4, sizes
    # (f) a relation whose lists are all entities
    assert any(kg.tail_list[r] == list(range(kg.E)) and kg.head_list[r] == list(range(kg.E)) for r in range(kg.R))
    # (g) duplicate training lines
    assert len(kg.train) > len(kg.uniq)
    # the untyped draw never divides by zero here
    assert all(len(v) < kg.E for v in kg.tails.values()) and all(len(v) < kg.E for v in kg.heads.values())
    assert all(len(v) < kg.R for v in kg.rels.values())
