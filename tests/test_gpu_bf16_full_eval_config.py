"""Config on bf16 tables, the full-entity evaluators: under set_bf16_evaluation("stored") rank_triples, validation_link_prediction(),
top_k_tails and top_k_heads stream the stored rows (kge_rank_triples_bf16, kge_topk_entities_bf16) -- the results of an fp32 Config
holding the widened parameters, as bytes, with no float32 view and the tables untouched.  Under "view" they fall back to the stored
rows when the view cannot be made, while link_prediction keeps raising.  Then the point of it in bytes, in a process of its own:
on a 262 144 x 64 table the stored path stays below half a view where the view path takes a view and a candidate table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_bf16_eval_config import B, N_BATCHES, bits, engine, same, triples

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def trained_pair():
    con = engine("bf16")
    for _ in range(2):
        con.train_step()
    fp32 = engine(None)
    fp32.set_parameters(con.get_parameters())
    return con, fp32


def full_entity_ops():
    _, _, test = triples()
    h, t, r = test[:, 0], test[:, 1], test[:, 2]
    return {
        "rank_triples": lambda c: c.rank_triples(h, t, r),
        "rank_triples, tail side": lambda c: c.rank_triples(h, t, r, test_head=False),
        "validation_link_prediction": lambda c: c.validation_link_prediction(),
        "top_k_tails": lambda c: c.top_k_tails(h, r, 10),
        "top_k_tails, filtered and typed": lambda c: c.top_k_tails(h, r, 10, filtered=True, type_constrained=True),
        "top_k_heads, filtered and typed": lambda c: c.top_k_heads(t, r, 10, filtered=True, type_constrained=True),
        "top_k_heads, k = 300": lambda c: c.top_k_heads(t, r, 300, filtered=True),
    }


def test_stored_mode_gives_the_fp32_results_and_makes_no_view():
    con, fp32 = trained_pair()
    con.set_bf16_evaluation("stored")
    fp32.set_bf16_evaluation("stored")          # no effect on fp32 tables
    before = bits(con)
    for name, op in full_entity_ops().items():
        got, want = op(con), op(fp32)
        assert same(got, want), (name, got, want)
        assert con._eval_view is None, name
        assert same(bits(con), before), name
    counts, metrics = con.rank_triples(*(triples()[2][:, i] for i in range(3)))
    assert counts[:, :, 0].any() and (counts[:, :, 1] <= counts[:, :, 0]).all() and 0.0 < metrics["r_filter_reci_rank"] <= 1.0
    # a view made earlier is neither used nor dropped by the stored path
    con.set_bf16_evaluation("view")
    con.rank_triples([0], [1], [0])
    view = con._eval_view
    assert view is not None
    con.set_bf16_evaluation("stored")
    con.rank_triples([0], [1], [0])
    assert con._eval_view is view


def test_view_mode_falls_back_to_the_stored_rows_when_the_view_cannot_be_made(monkeypatch, capsys):
    import openkeonspark_amd as pkg
    con, fp32 = trained_pair()
    assert con._bf16_evaluation == "view"
    asked = []

    def no_view():
        asked.append(1)
        raise con._eval_view_error(123456, "out of memory")
    monkeypatch.setattr(con, "_eval_table_ptrs", no_view)
    capsys.readouterr()
    for name, op in full_entity_ops().items():
        got, want = op(con), op(fp32)
        assert same(got, want), (name, got, want)
        assert con._eval_view is None, name
        said = capsys.readouterr().err.strip().splitlines()
        assert len(said) == 1 and "stored bf16 rows" in said[0], (name, said)        # one line saying so
    assert asked
    # the evaluators with no stored form keep raising, and name the ones that need no view
    for op in (lambda: con.link_prediction(), lambda: con.relation_prediction(), lambda: con.top_k_relations([0], [1], 2)):
        with pytest.raises(pkg.KgeError) as e:
            op()
        assert "rank_triples" in str(e.value) and "top_k_tails" in str(e.value) and "123456 bytes" in str(e.value)


CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import ctypes, json
import torch
from test_gpu_bf16_eval_config import B, N_BATCHES, engine, triples

ent, dim, n, k = 262144, 64, 100, 10
splits = triples(ent, n_train=B * N_BATCHES, n_eval=n)
con = engine("bf16", ent=ent, dim=dim, splits=splits)
h, t, r = splits[2][:, 0], splits[2][:, 1], splits[2][:, 2]

def workspace(reset):
    live, peak = ctypes.c_int64(), ctypes.c_int64()
    assert con.lib.kge_workspace_bytes(ctypes.byref(live), ctypes.byref(peak), reset) == 0
    return live.value, peak.value

out = dict(view_bytes=sum(x.numel() for x in con._tables) * 4, table_bytes=ent * dim * 4)
for mode in ("stored", "view"):          # stored first: the evaluators' workspaces begin empty
    con.set_bf16_evaluation(mode)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    live0, _ = workspace(1)
    counts, _ = con.rank_triples(h, t, r)
    ids, _ = con.top_k_tails(h, r, k)
    torch.cuda.synchronize()
    out[mode] = dict(torch=torch.cuda.max_memory_allocated() - base, workspace=workspace(0)[1] - live0,
                     view=con._eval_view is not None, counted=int(counts[:, :, 0].sum()), ids=int((ids >= 0).sum()))
print("RESULT " + json.dumps(out))
"""


def test_stored_mode_allocates_no_table_sized_buffer():
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    out = json.loads([l for l in run.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(out)
    view_bytes, table_bytes = out["view_bytes"], out["table_bytes"]
    assert view_bytes >= 67_000_000
    stored, view = out["stored"], out["view"]
    assert stored["counted"] > 0 and stored["ids"] == 100 * 10 and not stored["view"]
    assert stored["torch"] + stored["workspace"] < view_bytes // 2
    # the control: both measures see what they are meant to see when the view path runs
    assert view["view"] and view["torch"] >= view_bytes and view["workspace"] >= table_bytes
    assert (view["counted"], view["ids"]) == (stored["counted"], stored["ids"])
