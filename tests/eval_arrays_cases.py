"""Shared by the evaluation-from-arrays tests: the golden splits as arrays, the engine's evaluation arrays read back through
kge_eval_copy, and the type lists the reference's n_n() would generate, restated in a few lines (main_spark.py:209-290)."""
import os

import numpy as np

from conftest import GOLDEN

TRIPLE_ARRAYS = ("all", "all_t", "all_ht", "test", "valid")
TYPE_ARRAYS = ("head_lef", "head_rig", "tail_lef", "tail_rig", "head_type", "tail_type")


def read_split(d, name):
    tok = open(os.path.join(d, name)).read().split()
    a = np.asarray(tok[1:1 + 3 * int(tok[0])], dtype=np.int64).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()      # on disk: head, tail, relation


def read_kg(name):
    d = os.path.join(GOLDEN, name)
    first = lambda f: int(open(os.path.join(d, f)).readline())
    return dict(dir=d, E=first("entity2id.txt"), R=first("relation2id.txt"), train=read_split(d, "train2id.txt"),
                valid=read_split(d, "valid2id.txt"), test=read_split(d, "test2id.txt"))


def read_type_file(path, R):
    """type_constrain.txt as CSR (head_off, head_ids, tail_off, tail_ids), ids in file order, duplicates kept."""
    tok = [int(x) for x in open(path).read().split()]
    lists = [[[] for _ in range(R)] for _ in range(2)]
    p = 1
    for _ in range(tok[0]):
        for side in range(2):
            rel, n = tok[p], tok[p + 1]
            lists[side][rel] = tok[p + 2:p + 2 + n]
            p += 2 + n
    out = []
    for side in range(2):
        out.append(np.cumsum([0] + [len(x) for x in lists[side]]).astype(np.int64))
        out.append(np.asarray([e for x in lists[side] for e in x], dtype=np.int64))
    return tuple(out)


def n_n_lists(R, *splits):
    """{r: sorted(set(heads))}, {r: sorted(set(tails))} over the given (h, t, r) splits, for every relation."""
    h = np.concatenate([s[0] for s in splits]); t = np.concatenate([s[1] for s in splits]); r = np.concatenate([s[2] for s in splits])
    heads = {q: sorted(set(h[r == q].tolist())) for q in range(R)}
    tails = {q: sorted(set(t[r == q].tolist())) for q in range(R)}
    return heads, tails


def eval_array(L, name):
    nbytes = L.kge_eval_copy(name.encode(), None, 0)
    assert nbytes >= 0, name
    a = np.zeros(nbytes // 4, dtype=np.int32)
    assert L.kge_eval_copy(name.encode(), a.ctypes.data, nbytes) == nbytes
    return a.reshape(-1, 4) if name in TRIPLE_ARRAYS else a


def snapshot(L):
    """Every named evaluation array, the totals, and the type lists per relation as slices (where a list sits inside
    head_type / tail_type is the import's business: a file lists relations in its own order)."""
    out = {name: eval_array(L, name) for name in TRIPLE_ARRAYS + TYPE_ARRAYS}
    out["totals"] = np.array([L.getTestTotal(), L.getValidTotal(), L.getTripleTotal()])
    return out


def type_slices(snap):
    R = len(snap["head_lef"])
    return ({q: snap["head_type"][snap["head_lef"][q]:snap["head_rig"][q]].tolist() for q in range(R)},
            {q: snap["tail_type"][snap["tail_lef"][q]:snap["tail_rig"][q]].tolist() for q in range(R)})


def assert_same_triples(a, b):
    for k in TRIPLE_ARRAYS + ("totals",):
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k


def assert_same_bits(a, b):
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k


def file_config(d, threads=4):
    from openkeonspark_amd.Config import Config
    con = Config()
    con.set_in_path(d); con.set_work_threads(threads); con.set_bern(1); con.set_nbatches(7)
    con.init()
    con.init_link_prediction()
    return con


def array_config(kg, threads=4, **eval_kw):
    """init_from_arrays + init_evaluation_from_arrays over a read_kg() dictionary (or any with its keys)."""
    from openkeonspark_amd.Config import Config
    con = Config()
    con.set_work_threads(threads); con.set_bern(1); con.set_nbatches(7)
    con.init_from_arrays(kg["E"], kg["R"], *kg["train"])
    con.init_evaluation_from_arrays(kg["valid"], kg["test"], **eval_kw)
    return con
