"""The host half of candidate-list ranking over a sharded entity table: the dispatch of Config.rank_candidates_distributed with
one process, the refusals that need no process group, the driver's help text and the ctypes binding of
kge_rank_candidates_range against the header.  No GPU and no engine: the Config methods are called on a stand-in."""
import os
import re
import types

import pytest

from conftest import ROOT
from openkeonspark_amd import distribute_training as dt
from openkeonspark_amd.Config import Config, KgeError


def test_one_process_with_replicated_tables_is_rank_candidates():
    seen = []
    con = types.SimpleNamespace(_sharded=lambda name: False, world_size=1)
    con.rank_candidates = lambda *a: seen.append(a) or "result"
    assert Config.rank_candidates_distributed(con, [0], [1], [2], [3, 4], None, False) == "result"
    assert seen == [([0], [1], [2], [3, 4], None, False)]
    assert Config.rank_candidates_distributed(con, [0], [1], [2], head_candidates=[5]) == "result"
    assert seen[1] == ([0], [1], [2], None, [5], True)


def test_a_sharded_table_without_a_process_group_names_what_is_missing():
    con = types.SimpleNamespace(_sharded=lambda name: name == "ent_embeddings", world_size=2)
    for call in (lambda: Config.rank_candidates_distributed(con, [0], [1], [0], [2, 3]),
                 lambda: Config.rank_triples_sampled_distributed(con, [0], [1], [0], 5),
                 lambda: Config.validation_link_prediction_distributed(con, candidates=5)):
        with pytest.raises(KgeError, match="sharded across ranks needs the process group it was sharded over"):
            call()


def test_the_refusal_of_the_plain_methods_names_the_collectives():
    con = types.SimpleNamespace(_sharded=lambda name: True)
    with pytest.raises(KgeError) as e:
        Config._refuse_sharded_candidates(con, "rank_candidates")
    for name in ("rank_candidates_distributed", "rank_triples_sampled_distributed", "validation_link_prediction_distributed"):
        assert name in str(e.value)


def test_the_drivers_help_says_what_candidates_do_on_a_sharded_table(capsys):
    with pytest.raises(SystemExit):
        dt.parse_args(["--help"])
    helptext = " ".join(capsys.readouterr().out.split())
    entry = helptext[helptext.rindex("--early_stop_candidates EARLY_STOP_CANDIDATES"):]      # (the first is the usage line)
    entry = entry[:entry.index("--early_stop_candidates_seed")]
    assert "sharded across ranks" in entry and "validation_link_prediction_distributed" in entry
    assert "Not with" not in entry


def test_the_binding_has_the_headers_argument_list():
    """One ctypes type per parameter of the declaration in include/kge_mi355.h, pointers as void pointers, INT as int64."""
    import ctypes
    with open(os.path.join(ROOT, "include", "kge_mi355.h")) as f:
        header = f.read()
    decl = re.search(r"\bint kge_rank_candidates_range\((.*?)\);", header, re.S)
    assert decl, "kge_rank_candidates_range is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    names = [re.sub(r"\[.*\]", "", p).split()[-1].lstrip("*") for p in params]
    assert names == ["m", "tables", "row_lo", "rows", "d_query_rows", "d_h", "d_t", "d_r", "n", "d_tail_cand", "tail_stride",
                     "d_head_cand", "head_stride", "n_cand", "flags", "seed", "d_counts", "stream"]

    def kind(p):
        if "*" in p or "[" in p:
            return "pointer"
        return "uint64" if p.startswith("uint64_t") else "int64"
    want = [kind(p) for p in params]
    src = open(os.path.join(ROOT, "openkeonspark_amd", "_lib.py")).read()
    bound = re.search(r"L\.kge_rank_candidates_range\.argtypes = \[(.*?)\]", src, re.S)
    assert bound, "_lib.py does not bind kge_rank_candidates_range"
    got = []
    for a in (x.strip() for x in bound.group(1).split(",")):
        got.append({"i64": "int64", "ctypes.c_uint64": "uint64"}.get(a, "pointer" if a in ("vp", "tabs", "ctypes.POINTER(ModelDesc)") else a))
    assert got == want
    assert ctypes.sizeof(ctypes.c_uint64) == 8
