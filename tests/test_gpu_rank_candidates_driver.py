"""Training driver: early stop on validation MRR ranked against drawn candidate lists (--early_stop_candidates,
--early_stop_candidates_seed), by Config.validation_link_prediction(candidates=...)."""
import os

import pytest

from conftest import GOLDEN
from openkeonspark_amd import distribute_training as dt
from openkeonspark_amd import rank_eval

pytestmark = pytest.mark.gpu


def run(tmp_path, name, extra, kg="kg_small"):
    out = str(tmp_path / name)
    args = dt.parse_args(["--input_path", os.path.join(GOLDEN, kg), "--output_path", out, "--embedding_dimension", "16",
                          "--n_mini_batches", "2", "--alpha", "0.0", "--train_times", "40", "--early_stop_patience", "2",
                          "--debug", "1"] + extra)
    return out, dt.main_fun(args)


@pytest.fixture
def candidate_calls(monkeypatch):
    """Every kge_rank_candidates call Config makes in a run: (triples, candidates, flags, seed)."""
    calls = []
    real = rank_eval.rank_candidates_device

    def spy(con, dev, tail, head, n_cand, flags, seed, first=0, into=None):
        calls.append((int(dev.shape[1]), n_cand, flags, seed))
        return real(con, dev, tail, head, n_cand, flags, seed, first, into)
    monkeypatch.setattr(rank_eval, "rank_candidates_device", spy)
    return calls


def test_early_stop_on_mrr_against_drawn_candidates(tmp_path, capsys, candidate_calls):
    out, con = run(tmp_path, "cand", ["--early_stop_metric", "mrr", "--early_stop_candidates", "20"])
    text = capsys.readouterr().out           # lr = 0: the metric cannot improve -> stops after `patience` checks
    assert "Early Stop Check (mrr)" in text and "mrr early stop" in text
    assert os.path.exists(os.path.join(out, "stop.txt")) and con.global_step == 3 * con.nbatches
    # every check: all validation triples, 20 drawn candidates, filtered, tail side only (--test_head 0), seed 0
    assert candidate_calls == [(con.validTotal, 20, 1 | 2 | 8, 0)] * 3
    checks = [l for l in text.splitlines() if l.startswith("[ Early Stop Check")]
    now = [float(l.split("now")[1]) for l in checks]
    assert len(now) == 3 and now[0] == now[1] == now[2] and 0.0 < now[0] <= 1.0
    counts, metrics = con.validation_link_prediction(test_head=False, candidates=20, seed=0)
    assert counts.shape == (con.validTotal, 2, 2) and counts[:, 0, 0].any() and not counts[:, 1].any()
    assert abs(now[0] - metrics["r_filter_reci_rank"]) < 1e-9
    # twenty candidates are not the whole table: the full ranking gives another value
    assert abs(now[0] - con.validation_link_prediction(test_head=False)[1]["r_filter_reci_rank"]) > 1e-6


def test_seed_sample_head_side_and_typed_lists(tmp_path, capsys, candidate_calls):
    out, con = run(tmp_path, "cand2", ["--early_stop_metric", "hits10", "--early_stop_candidates", "30", "--early_stop_candidates_seed", "5",
                                       "--early_stop_rank_triples", "9", "--test_head", "1", "--type_constrained_sampling", "1"])
    text = capsys.readouterr().out
    assert candidate_calls and all(c == (9, 30, 1 | 2 | 4, 5) for c in candidate_calls)
    met = con.validation_link_prediction(test_head=True, sample=9, candidates=30, seed=5, type_constrained=True)[1]
    now = float([l for l in text.splitlines() if l.startswith("[ Early Stop Check")][0].split("now")[1])
    assert abs(now - (met["r_filter_tot"] + met["l_filter_tot"]) / 2) < 1e-9
