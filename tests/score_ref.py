"""The predict op's score from its definition, in plain numpy fp64, and "axis" tables on which the fp32 score is an integer.

scores() restates the four predict ops (TransE.py:53-58, TransH.py:71-82, TransR.py:77-87, TransD.py:86-98) with
l2n(x) = x * rsqrt(max(sum x^2, 1e-12)): TransE the MEAN over the dimension of |l2n(h) + l2n(r) - l2n(t)|, the projecting
models the SUM, their transfers as in tests/torch_ref.py.  TransR has two contracts (include/kge_mi355.h): kge_predict
projects every triple of a call by the matrix of r[0] ("predict"), the rankers, top-k and relation prediction project each
triple by its own relation's matrix ("own_matrix").  tests/test_score_ref.py pins scores() to the C oracle.

exact_tables() builds tables on which every intermediate value of the forward is exactly representable in fp32 -- every row
is zero or a power of two on ONE axis, so sums of squares are powers of four, 1/sqrt of them is exact, normalised rows are
+-unit vectors and the score is a small integer: no summation order, fma contraction or reduction tree can change a bit.
exact_scores() derives that integer from the tables by integer arithmetic on (axis, sign) pairs, never touching l2n."""
import numpy as np

MODELS = ("transe", "transh", "transd", "transr")
TABLES = {"transe": ("ent_embeddings", "rel_embeddings"),
          "transh": ("ent_embeddings", "rel_embeddings", "normal_vectors"),
          "transr": ("ent_embeddings", "rel_embeddings", "transfer_matrix"),
          "transd": ("ent_embeddings", "rel_embeddings", "rel_transfer", "ent_transfer")}
RUNGS = ((16, 16, 1), (32, 16, 2), (64, 16, 4), (128, 32, 4), (256, 64, 4), (512, 64, 8), (1024, 64, 16))   # (widths up to, L, C): csrc/team_shape.hpp
CHUNK = 4096


def rung_of(D):
    """(L, C) of width D: lane l of a team holds elements l, l + L, ..., l + (C - 1) L (csrc/team.hpp)."""
    for top, L, C in RUNGS:
        if D <= top:
            return L, C
    raise ValueError("no rung for width %d" % D)


def l2n(x):
    ss = (x * x).sum(-1, keepdims=True)
    one = x.dtype.type(1)
    return x * (one / np.sqrt(np.maximum(ss, x.dtype.type(1e-12))))


def _chunk_scores(model, P, h, t, r, mr, De, Dr):
    ent, rel = P["ent_embeddings"], P["rel_embeddings"]
    if model == "transe":
        ph, pt = ent[h], ent[t]
    elif model == "transh":
        w = l2n(P["normal_vectors"][r])
        ph = ent[h] - (ent[h] * w).sum(-1, keepdims=True) * w
        pt = ent[t] - (ent[t] * w).sum(-1, keepdims=True) * w
    elif model == "transd":
        et, rp = P["ent_transfer"], P["rel_transfer"][r]
        ph = ent[h] + (ent[h] * et[h]).sum(-1, keepdims=True) * rp
        pt = ent[t] + (ent[t] * et[t]).sum(-1, keepdims=True) * rp
    else:
        ph = np.empty((len(h), Dr), ent.dtype)
        pt = np.empty((len(h), Dr), ent.dtype)
        for q in np.unique(mr).tolist():
            m = mr == q
            M = P["transfer_matrix"][q].reshape(De, Dr)
            ph[m] = ent[h[m]] @ M
            pt[m] = ent[t[m]] @ M
    e = np.abs(l2n(ph) + l2n(rel[r]) - l2n(pt))
    return e.mean(-1) if model == "transe" else e.sum(-1)


def scores(model, params, h, t, r, De, Dr, variant="predict", dtype=np.float64):
    """The score of every triple (h[i], t[i], r[i]) from the definition, evaluated in `dtype` (fp64: the reference; fp32: what
    a plain single-precision evaluation of the same formula gives, for comparison).  variant: TransR's matrix, see above."""
    assert model in MODELS and variant in ("predict", "own_matrix")
    h, t, r = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (h, t, r))
    P = {k: np.asarray(params[k]).astype(dtype, copy=False) for k in TABLES[model]}
    out = np.empty(len(h), dtype)
    mr = r if variant == "own_matrix" or len(r) == 0 else np.full_like(r, r[0])
    for lo in range(0, len(h), CHUNK):
        s = slice(lo, lo + CHUNK)
        out[s] = _chunk_scores(model, P, h[s], t[s], r[s], mr[s], De, Dr)
    return out


def fp32_error(model, params, h, t, r, De, Dr, want, variant="predict"):
    """Worst |fp32 numpy evaluation - want| / want over the triples: the yardstick a kernel's error is reported beside."""
    got = scores(model, params, h, t, r, De, Dr, variant, dtype=np.float32).astype(np.float64)
    return float((np.abs(got - want) / want).max())


# --------------------------------------------------------------------------------------------------------------------------
# axis tables
# --------------------------------------------------------------------------------------------------------------------------
SCALES = (0.5, 1.0, 2.0, 4.0)          # squares 0.25, 1, 4, 16: 1/sqrt of each is exact


def special_axes(D):
    """Axes where a wrong team shape shows: the last element of the row, the first and last element of the last slab of its
    rung (elements [L (C - 1), L C)), the last element below that slab, the ends of the first slab, and the same for every
    smaller rung (a width sent to a rung too small loses exactly the elements beyond that rung's L C)."""
    ax = {0, D - 1, D - 2, (D - 1) // 2}
    for top, L, C in RUNGS:
        ax |= {L - 1, L, L * (C - 1) - 1, L * (C - 1), L * C - 1, L * C, L * C + 1}
        if D <= top:
            break
    return sorted(a for a in ax if 0 <= a < D)


def entity_axes(E, D):
    """Row j lives on axis j % D, except every fourth row, which walks through special_axes(D)."""
    ax = np.arange(E) % D
    sp = np.asarray(special_axes(D))
    j = np.arange(3, E, 4)
    ax[j] = sp[(j // 4) % len(sp)]
    return ax


def _axis_rows(axes, values, D):
    out = np.zeros((len(axes), D), np.float32)
    out[np.arange(len(axes)), axes] = values
    return out


def transr_columns(R, De, Dr):
    """(col [R, De], sign [R, De]): row i of relation q's matrix holds sign at column col and zeros elsewhere.  The columns
    stride over all of Dr (every 128-column block of the projection is hit when De rows reach it), and every row with
    i % 4 == 1 shares the column of row i - 1."""
    i = np.arange(De)
    stride = max(1, Dr // max(De, 1))
    base = (i - (i % 4 == 1)) * stride
    q = np.arange(R)[:, None]
    col = (base[None, :] + 17 * q + Dr - 1) % Dr
    sign = np.where((i[None, :] + q) % 3 == 0, -1, 1)
    return col, sign


def exact_tables(model, E, R, De, Dr):
    """Axis tables (float32) for `model`; see the module docstring.  TransE / TransH / TransD need De == Dr."""
    assert model in MODELS and (model == "transr" or De == Dr)
    j, q = np.arange(E), np.arange(R)
    ax = entity_axes(E, De)
    val = np.asarray(SCALES)[(j // 3) % 4] * np.where(j % 5 == 2, -1.0, 1.0)
    P = {"ent_embeddings": _axis_rows(ax, val, De)}
    sp = np.asarray(special_axes(Dr))
    rax = np.where(q % 3 == 1, Dr - 1, sp[(q // 3 + 1) % len(sp)])
    rval = np.where(q % 3 == 0, 0.0, np.asarray(SCALES)[(q + 1) % 4] * np.where(q % 2 == 0, -1.0, 1.0))   # q % 3 == 0: the zero row
    P["rel_embeddings"] = _axis_rows(rax, rval, Dr)
    if model == "transh":        # the projection zeroes the rows on the normal's axis and keeps every other row
        nax = np.where(q % 3 == 0, Dr - 1, np.where(q % 3 == 1, 0, sp[(q // 3 + 2) % len(sp)]))
        P["normal_vectors"] = _axis_rows(nax, np.asarray(SCALES)[q % 4] * np.where(q % 2 == 1, -1.0, 1.0), Dr)
    elif model == "transd":
        # x + (x . x_p) r_p stays on one axis when r_p lies on x's axis or x . x_p == 0.  Every r_p lies on the LAST axis; a row on the
        # last axis has x_p = p there, every other row has its x_p on the next axis (a non-zero row that the dot product must null).
        # x (1 + p q) with p in {1, -1, 0} and q in {1, -1, 3, 0, -3}: 1 + p q in {2, 0, 4, -2, 1}, a power of two or zero.
        P["rel_transfer"] = _axis_rows(np.full(R, Dr - 1), np.asarray([1.0, -1.0, 3.0, 0.0, -3.0])[q % 5], Dr)
        last = ax == De - 1
        p = np.where(last, np.asarray([1.0, -1.0, 0.0])[(j // 4) % 3], np.where(j % 2 == 0, 1.0, -2.0))
        P["ent_transfer"] = _axis_rows(np.where(last, De - 1, (ax + 1) % De), p, De)
    elif model == "transr":
        col, sign = transr_columns(R, De, Dr)
        M = np.zeros((R, De, Dr), np.float32)
        M[q[:, None], np.arange(De)[None, :], col] = sign
        P["transfer_matrix"] = M.reshape(R, De * Dr)
    return P


def _units(rows, scale=1):
    """(axis, integer value * scale) of every row; a zero row has value 0.  Asserts the single-axis shape."""
    rows = np.asarray(rows)
    assert ((rows != 0).sum(-1) <= 1).all(), "not an axis table"
    ax = np.abs(rows).argmax(-1)
    v = rows[np.arange(len(rows)), ax].astype(np.float64) * scale
    assert (v == np.rint(v)).all()
    return ax, v.astype(np.int64)


def _l1(terms):
    """sum over axes of |sum of the coefficients on that axis| for per-triple lists of (axis, coefficient) terms."""
    total = np.zeros(len(terms[0][0]), np.int64)
    for i, (a, c) in enumerate(terms):
        first = np.ones(len(a), bool)
        for b, _ in terms[:i]:
            first &= b != a
        s = c.copy()
        for b, d in terms[i + 1:]:
            s += np.where(b == a, d, 0)
        total += np.where(first, np.abs(s), 0)
    return total


def exact_scores(model, params, h, t, r, De, Dr, variant="predict"):
    """The score of every triple on axis tables, as float32, from integer arithmetic: a normalised row is (axis, sign), a
    projection maps (axis, sign) to (axis', sign') or to zero, and the L1 distance of three signed unit vectors is counted.
    TransE divides the count by np.float32(De), one IEEE division."""
    assert model in MODELS and variant in ("predict", "own_matrix")
    h, t, r = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (h, t, r))
    eax, ev = _units(params["ent_embeddings"], 2)         # values in halves
    rax, rv = _units(params["rel_embeddings"], 2)

    def side(e):
        ax, v = eax[e], ev[e]
        if model == "transh":
            nax, nv = _units(params["normal_vectors"], 2)
            return ax, np.where((nv[r] != 0) & (nax[r] == ax), 0, v)
        if model == "transd":
            pax, pv = _units(params["ent_transfer"])
            qax, qv = _units(params["rel_transfer"])
            a = np.where(pax[e] == ax, v * pv[e], 0)          # (x . x_p), in halves
            assert ((a == 0) | (qv[r] == 0) | (qax[r] == ax)).all(), "x + (x . x_p) r_p leaves its axis"
            return ax, v + a * qv[r]
        if model == "transr":
            M = np.asarray(params["transfer_matrix"]).reshape(-1, De, Dr)
            assert ((M != 0).sum(-1) == 1).all() and (np.abs(M).max(-1) == 1).all()
            col, sign = np.abs(M).argmax(-1), np.rint(M.sum(-1)).astype(np.int64)
            mr = r if variant == "own_matrix" or len(r) == 0 else np.full_like(r, r[0])
            return col[mr, ax], v * sign[mr, ax]
        return ax, v

    (ha, hv), (ta, tv) = side(h), side(t)
    n = _l1([(ha, np.sign(hv)), (rax[r], np.sign(rv[r])), (ta, -np.sign(tv))])
    s = n.astype(np.float32)
    return s / np.float32(De) if model == "transe" else s


# --------------------------------------------------------------------------------------------------------------------------
# random tables, made-up graphs and the evaluators' definitions (shared by the CPU and the GPU tests, so that what the CPU test
# asserts about a seed is what the GPU test runs)
# --------------------------------------------------------------------------------------------------------------------------
BAND = 2e-5          # two fp32 scores, each within 1e-5 of fp64, may swap when their fp64 values are this close (relative)
MAX_ASIDE = 0.05     # share of queries the random comparisons may set aside
EVAL_WIDTHS = (7, 24, 64, 100, 200, 260, 520, 1024)          # one width per rung (and a second on the widest)
EVAL_TRANSR = ((8, 8), (8, 260), (33, 50))
EVAL_CASES = [(m, d, d) for m in ("transe", "transh", "transd") for d in EVAL_WIDTHS] + [("transr", de, dr) for de, dr in EVAL_TRANSR]
EVAL_R = 5
EVAL_E_EXACT = 300


def eval_entities(kind, Dr):
    """Entities of an evaluation case.  Random tables: scores concentrate as the width grows (their relative spread falls like
    1 / sqrt(D)), so more of the candidates land within BAND of one another in fp64 itself; 120 candidates keep the set-aside
    share under MAX_ASIDE up to width 100, 60 beyond (tests/test_score_ref.py asserts it for every case)."""
    return EVAL_E_EXACT if kind == "exact" else (120 if Dr <= 100 else 60)


def seed_of(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def random_tables(model, E, R, De, Dr, seed, scale=1.0):
    """Xavier-sized normal tables (stddev sqrt(2.6 / (rows + cols)), as the engine initialises them) times `scale`, float32."""
    rng = np.random.default_rng(seed)
    shapes = {"ent_embeddings": (E, De), "rel_embeddings": (R, Dr), "normal_vectors": (R, Dr), "transfer_matrix": (R, De * Dr),
              "rel_transfer": (R, Dr), "ent_transfer": (E, De)}
    return {k: (rng.standard_normal(shapes[k]) * np.sqrt(2.6 / sum(shapes[k])) * scale).astype(np.float32) for k in TABLES[model]}


def eval_graph(E, R, seed, n_test=60, n_valid=30):
    """Made-up train / valid / test triples as (h, t, r) array triples.  The training set holds, for every evaluation triple,
    other tails of its (h, r), other heads of its (t, r) and other relations of its (h, t), so that every filter bites;
    duplicates and a triple with h == t are kept."""
    rng = np.random.default_rng(seed)
    draw = lambda n: [rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)]
    test, valid, extra = draw(n_test), draw(n_valid), draw(150)
    test[1][0] = test[0][0]                                   # h == t
    valid[0][:2], valid[1][:2], valid[2][:2] = test[0][:2], test[1][:2], test[2][:2]      # two triples in both splits
    ev = [np.concatenate([test[i], valid[i]]) for i in range(3)]
    rows = [np.stack(extra, 1)]
    for k in range(4):
        rows.append(np.stack([ev[0], rng.integers(0, E, len(ev[0])), ev[2]], 1))
        rows.append(np.stack([rng.integers(0, E, len(ev[0])), ev[1], ev[2]], 1))
    rows.append(np.stack([ev[0], ev[1], rng.integers(0, R, len(ev[0]))], 1))
    train = np.concatenate(rows)
    train = np.concatenate([train, train[:20]])              # duplicates
    return dict(E=E, R=R, train=(train[:, 0].copy(), train[:, 1].copy(), train[:, 2].copy()), valid=tuple(valid), test=tuple(test))


def known_triples(graph):
    return {(int(h), int(t), int(r)) for split in ("train", "valid", "test") for h, t, r in zip(*graph[split])}


def made_up_type_lists(E, R, seed):
    """CSR (head_off, head_ids, tail_off, tail_ids): about 60 % of the entities per list; relation 1 has two empty lists."""
    rng = np.random.default_rng(seed)
    out = []
    for side in range(2):
        lists = [np.sort(rng.choice(E, int(0.6 * E), replace=False)) if q != 1 else np.zeros(0, np.int64) for q in range(R)]
        out += [np.cumsum([0] + [len(x) for x in lists]).astype(np.int64), np.concatenate(lists).astype(np.int64)]
    return tuple(out)


def derived_type_lists(graph):
    """What derive_types=True gives: every relation's distinct heads and distinct tails over train + valid + test."""
    h, t, r = (np.concatenate([graph[s][i] for s in ("train", "valid", "test")]) for i in range(3))
    out = []
    for ids in (h, t):
        lists = [np.unique(ids[r == q]) for q in range(graph["R"])]
        out += [np.cumsum([0] + [len(x) for x in lists]).astype(np.int64), np.concatenate(lists).astype(np.int64)]
    return tuple(out)


def type_masks(lists, E, R):
    """-> (head [R, E] bool, tail [R, E] bool) membership of the CSR lists."""
    masks = []
    for off, ids in ((lists[0], lists[1]), (lists[2], lists[3])):
        m = np.zeros((R, E), bool)
        for q in range(R):
            m[q, ids[off[q]:off[q + 1]]] = True
        masks.append(m)
    return tuple(masks)


class Evaluators:
    """The evaluators' results from their definitions (include/kge_mi355.h) over a score function score(h, t, r) -> array:
    exact_scores on axis tables, scores (fp64, own_matrix) on random ones.  Candidate scores are cached per query."""

    def __init__(self, score, graph, lists=None):
        self.score, self.E, self.R = score, graph["E"], graph["R"]
        self.known = known_triples(graph)
        self.known_tails, self.known_heads = {}, {}
        for h, t, r in self.known:
            self.known_tails.setdefault((h, r), set()).add(t)
            self.known_heads.setdefault((t, r), set()).add(h)
        self.head_type, self.tail_type = type_masks(lists, self.E, self.R) if lists is not None else (np.zeros((self.R, self.E), bool),) * 2
        self.cache = {}

    def entity_scores(self, fixed, r, head):
        """(scores of every entity as the head of (?, r, fixed) / tail of (fixed, r, ?), known mask, typed mask)"""
        key = (int(fixed), int(r), bool(head))
        if key not in self.cache:
            ar, fx, rr = np.arange(self.E), np.full(self.E, fixed), np.full(self.E, r)
            s = self.score(ar, fx, rr) if head else self.score(fx, ar, rr)
            known = np.zeros(self.E, bool)
            known[list((self.known_heads if head else self.known_tails).get(key[:2], ()))] = True
            self.cache[key] = (np.asarray(s), known, (self.head_type if head else self.tail_type)[key[1]])
        return self.cache[key]

    def relation_scores(self, h, t):
        key = (int(h), int(t))
        if key not in self.cache:
            s = self.score(np.full(self.R, h), np.full(self.R, t), np.arange(self.R))
            known = np.array([(key[0], key[1], q) in self.known for q in range(self.R)])
            self.cache[key] = (np.asarray(s), known, self.head_type[:, key[0]] & self.tail_type[:, key[1]])
        return self.cache[key]

    @staticmethod
    def _four(s, target, known, typed, band):
        below = s < s[target]                       # the reference's strict `<`
        below[target] = False
        near = np.abs(s - s[target]) <= band * abs(s[target])
        near[target] = False
        return [below.sum(), (below & ~known).sum(), (below & typed).sum(), (below & typed & ~known).sum()], bool(band and near.any())

    def rank_counts(self, h, t, r, band=0.0):
        """-> (counts int64 [n, 2, 4]: side 0 tail / side 1 head; raw, filtered, typed, typed + filtered, and aside bool [n, 2]:
        a candidate's score lies within `band` (relative) of the target's)."""
        counts, aside = np.zeros((len(h), 2, 4), np.int64), np.zeros((len(h), 2), bool)
        for i, (a, b, q) in enumerate(zip(h, t, r)):
            for side in (0, 1):
                s, known, typed = self.entity_scores(a if side == 0 else b, q, side == 1)
                counts[i, side], aside[i, side] = self._four(s, b if side == 0 else a, known, typed, band)
        return counts, aside

    def relation_counts(self, h, t, r, band=0.0):
        counts, aside = np.zeros((len(h), 4), np.int64), np.zeros(len(h), bool)
        for i, (a, b, q) in enumerate(zip(h, t, r)):
            s, known, typed = self.relation_scores(a, b)
            counts[i], aside[i] = self._four(s, q, known, typed, band)
        return counts, aside

    @staticmethod
    def select(s, eligible, k, band=0.0):
        """The k best by ascending (score, id) among the eligible -> (ids int64 [k] padded with -1, scores [k] padded with
        +inf, aside: the gap between the k-th and the (k+1)-th eligible score is within `band`, relative)."""
        ids = np.nonzero(eligible)[0]
        ids = ids[np.lexsort((ids, s[ids]))]
        aside = bool(band and len(ids) > k and s[ids[k]] - s[ids[k - 1]] <= band * abs(s[ids[k - 1]]))
        ids = ids[:k]
        out_ids, out_s = np.full(k, -1, np.int64), np.full(k, np.inf, np.asarray(s).dtype)
        out_ids[:len(ids)], out_s[:len(ids)] = ids, s[ids]
        return out_ids, out_s, aside

    def top_k_entities(self, fixed, r, head, k, filtered=False, band=0.0):
        rows = []
        for f, q in zip(fixed, r):
            s, known, _ = self.entity_scores(f, q, head)
            rows.append(self.select(s, ~known if filtered else np.ones(self.E, bool), k, band))
        return np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows]), np.array([x[2] for x in rows])

    def top_k_relations(self, h, t, k, filtered=False, band=0.0):
        rows = []
        for a, b in zip(h, t):
            s, known, _ = self.relation_scores(a, b)
            rows.append(self.select(s, ~known if filtered else np.ones(self.R, bool), k, band))
        return np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows]), np.array([x[2] for x in rows])


def eval_case(model, De, Dr, kind):
    """The engine-independent half of an evaluation case -> dict(graph, params, lists, ev): kind "exact" = axis tables scored
    by exact_scores, "random" = random tables (x 3) scored by scores() in fp64; TransR by each relation's own matrix."""
    E, R = eval_entities(kind, Dr), EVAL_R
    graph = eval_graph(E, R, seed_of("graph", kind))
    lists = made_up_type_lists(E, R, seed_of("types", kind))
    if kind == "exact":
        params = exact_tables(model, E, R, De, Dr)
        score = lambda h, t, r: exact_scores(model, params, h, t, r, De, Dr, "own_matrix")
    else:
        params = random_tables(model, E, R, De, Dr, seed_of("tables", model, De, Dr), 3.0)
        p64 = {k: v.astype(np.float64) for k, v in params.items()}
        score = lambda h, t, r: scores(model, p64, h, t, r, De, Dr, "own_matrix")
    return dict(graph=graph, params=params, lists=lists, ev=Evaluators(score, graph, lists), score=score)


def eval_queries(graph):
    """The triples the rank tests rank: test + valid, and the top-k queries (fixed entity, relation) / (h, t) taken from them."""
    h, t, r = (np.concatenate([graph["test"][i], graph["valid"][i]]) for i in range(3))
    return h, t, r


RANDOM_K = (1, 10)           # top-k entities on random tables
RANDOM_K_REL = (1, 3)        # top-k relations (of EVAL_R) on random tables
