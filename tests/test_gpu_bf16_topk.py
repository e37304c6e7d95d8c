"""kge_topk_entities_bf16 (include/kge_mi355.h, "Evaluation on bf16 tables"): every id and every score bit of kge_topk_entities on
the widened tables, padding and NaN order included, from the stored bf16 rows -- one width per rung of csrc/team_shape.hpp,
E = 1500 (two candidate slices, the merge stage, a ragged slice), 40 queries of mixed sides and relations with duplicates, k from 1
to 1024, every flag set, with the inverse-norm table and without ("topk_table_max_bytes" = 0)."""
import numpy as np
import pytest

import bf16_eval_rig as rig
import bf16_full_eval_rig as full

pytestmark = pytest.mark.gpu

E, NQ = 1500, 40
WIDTHS = rig.MULTIPLE_OF_8_PER_RUNG
KS = (1, 7, 64, 1024)
FILTERED, TYPED = 1, 2


def queries(rows=None):
    """(fixed, relation, head side) of 40 queries taken from the evaluation triples, so that the filter bites: tails of (h, r) and
    heads of (t, r) alternating in runs, two queries repeated; with `rows`, family (a)'s zero and tiny rows are queried too."""
    h, t, r = full.triples(E, NQ)
    head = ((np.arange(NQ) // 3) % 2).astype(np.int32)
    fixed = np.where(head == 1, t, h)
    rel = r.copy()
    for x in (fixed, rel, head):
        x[NQ - 2], x[NQ - 3] = x[1], x[4]
    if rows is not None:
        fixed[6], fixed[9] = rows["zero"], rows["tiny"]
    assert len(set(rel.tolist())) == full.R and 0 < head.sum() < NQ
    return tuple(rig.dev(x, np.int32) for x in (fixed, rel, head))


def compare(tabs, q, ks):
    seen_padding = seen_filter = False
    for k in ks:
        plain = None
        for flags in (0, FILTERED, TYPED, FILTERED | TYPED):
            rc32, ids32, bits32 = full.topk(tabs, *q, k, flags, bf16=False)
            assert rc32 == 0
            for budget in (full.TOPK_TABLE_DEFAULT, 0):
                with full.Options(topk_table_max_bytes=budget):
                    rc, ids, bits = full.topk(tabs, *q, k, flags)
                assert rc == 0, (k, flags, budget, rc)
                assert np.array_equal(ids, ids32), (k, flags, budget, full.first_diff(ids, ids32))
                assert np.array_equal(bits, bits32), (k, flags, budget, full.first_diff(bits, bits32))
            plain = ids32 if flags == 0 else plain
            seen_padding |= bool((ids32 == -1).any())
            seen_filter |= flags == FILTERED and not np.array_equal(ids32, plain)
        assert (plain[NQ - 2] == plain[1]).all() and (plain[NQ - 3] == plain[4]).all()      # duplicates select alike
    return seen_padding, seen_filter


@pytest.mark.parametrize("D", WIDTHS)
def test_ids_and_score_bits_are_the_fp32_kernels_on_the_widened_tables(D):
    con = full.import_graph(E)
    tabs, rows = full.special_tables(E, D, NQ)
    padding, filtered = compare(tabs, queries(rows), KS)
    # relation 1 has empty type lists and a type list holds 60 % of 1500 entities: k = 1024 pads; known triples were dropped
    assert padding and filtered
    # the inf row's and the NaN row's scores are NaN, which sorts after every number: 1498 numbers keep them out of any k
    rc, ids, bits = full.topk(tabs, *queries(rows), 1024, 0)
    assert rc == 0 and not np.isin(ids, [rows["nan"], rows["inf"]]).any()
    del con


def test_near_tie_tables_compare_nearly_every_score_and_order_ties_by_id():
    D = 24
    con = full.import_graph(E)
    tabs = full.tie_tables(E, D)
    q = queries()
    compare(tabs, q, (1024,))
    rc, ids, bits = full.topk(tabs, *q, 1024, 0)
    scores = bits.view(np.float32)
    assert rc == 0 and (np.diff(scores, axis=1) >= 0).all()
    tied = np.diff(scores, axis=1) == 0
    assert tied.sum() > 1000 and (np.diff(ids, axis=1)[tied] > 0).all()
    del con


def test_errors_are_the_fp32_calls_and_leave_the_outputs_untouched():
    import torch
    con = full.import_graph(E)
    D, k = 24, 7
    tabs, rows = full.special_tables(E, D, NQ)
    f, r, hd = queries(rows)
    out = (torch.full((NQ, k), full.FILL, dtype=torch.int32, device="cuda"), torch.full((NQ, k), float(full.FILL), dtype=torch.float32, device="cuda"))
    untouched = lambda: bool((out[0] == full.FILL).all().item() and (out[1] == float(full.FILL)).all().item())

    def call(bf16, f=f, r=r, hd=hd, k=k, flags=FILTERED, **kw):
        return full.topk(tabs, f, r, hd, k, flags, bf16=bf16, out=out, **kw)[0]
    for kw in (dict(f=None), dict(r=None), dict(hd=None), dict(n=-1), dict(k=0), dict(k=1025), dict(flags=4)):
        assert call(True, **kw) == call(False, **kw) == rig.KGE_ERR_BAD_ARG and untouched(), kw
    for kw in (dict(ent=None), dict(rel=None)):
        assert call(True, **kw) == rig.KGE_ERR_BAD_ARG and untouched(), kw
    assert call(True, n=0) == call(False, n=0) == 0 and untouched()
    for desc in (rig.desc(E, full.R, 12), rig.desc(E, full.R, 1032), rig.desc(E, full.R, D, model=1), rig.desc(E, full.R, D, 8)):
        assert call(True, d=desc) == rig.KGE_ERR_UNSUPPORTED and untouched(), (desc.model, desc.ent_dim)
    del con
