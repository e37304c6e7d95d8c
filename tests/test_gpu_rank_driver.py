"""Training driver: early stop on validation MRR / Hits@10 (--early_stop_metric, --early_stop_rank_triples), ranked by
Config.validation_link_prediction; the default accuracy criterion is unchanged."""
import os

import pytest

from conftest import GOLDEN
from openkeonspark_amd import distribute_training as dt
from openkeonspark_amd.Config import Config

pytestmark = pytest.mark.gpu


def run(tmp_path, name, extra, kg="kg_small"):
    out = str(tmp_path / name)
    args = dt.parse_args(["--input_path", os.path.join(GOLDEN, kg), "--output_path", out, "--embedding_dimension", "16",
                          "--n_mini_batches", "2", "--alpha", "0.0", "--train_times", "40", "--early_stop_patience", "2",
                          "--debug", "1"] + extra)
    return out, dt.main_fun(args)


@pytest.fixture
def ranking_calls(monkeypatch):
    """Every validation_link_prediction call of a run: (test_head, sample, rows ranked)."""
    calls = []
    real = Config.validation_link_prediction

    def spy(self, test_head=True, sample=0):
        counts, metrics = real(self, test_head=test_head, sample=sample)
        calls.append((test_head, sample, counts.shape[0]))
        return counts, metrics
    monkeypatch.setattr(Config, "validation_link_prediction", spy)
    return calls


@pytest.mark.parametrize("metric", ["mrr", "hits10"])
def test_ranking_early_stop(tmp_path, capsys, ranking_calls, metric):
    out, con = run(tmp_path, metric, ["--early_stop_metric", metric])
    text = capsys.readouterr().out           # lr = 0: neither the metric nor the loss can improve -> stops after `patience` checks
    assert "Early Stop Check (%s)" % metric in text and "Early Stop Check (Accuracy)" not in text
    assert "%s early stop" % metric in text          # the ranking criterion, not the loss criterion, ended the run
    assert os.path.exists(os.path.join(out, "stop.txt")) and con.global_step < 40 * con.nbatches
    # the first check sets the best value, the next `patience` checks do not improve on it
    assert len(ranking_calls) == 3 and con.global_step == 3 * con.nbatches
    assert all(c == (False, 0, con.validTotal) for c in ranking_calls)          # --test_head 0: the tail side, every validation triple
    checks = [l for l in text.splitlines() if l.startswith("[ Early Stop Check")]
    assert len(checks) == 3
    now = [float(l.split("now")[1]) for l in checks]
    assert now[0] == now[1] == now[2] and 0.0 < now[0] <= 1.0
    want = con.validation_link_prediction(test_head=False)[1]["r_filter_reci_rank" if metric == "mrr" else "r_filter_tot"]
    assert abs(now[0] - want) < 1e-9


def test_default_metric_is_the_accuracy_path(tmp_path, capsys, ranking_calls):
    out, con = run(tmp_path, "acc", ["--early_stop_metric", "accuracy"])
    text = capsys.readouterr().out
    assert "Early Stop Check (Accuracy)" in text and "early stop" in text
    assert os.path.exists(os.path.join(out, "stop.txt")) and con.global_step < 40 * con.nbatches
    assert not ranking_calls
    assert dt.parse_args([]).early_stop_metric == "accuracy" and dt.parse_args([]).early_stop_rank_triples == 0


def test_rank_triples_sample_and_head_side(tmp_path, capsys, ranking_calls):
    out, con = run(tmp_path, "sample", ["--early_stop_metric", "mrr", "--early_stop_rank_triples", "5", "--test_head", "1"])
    text = capsys.readouterr().out
    assert "Early Stop Check (mrr)" in text
    assert ranking_calls and all(c == (True, 5, 5) for c in ranking_calls)
    met = con.validation_link_prediction(test_head=True, sample=5)[1]
    now = float([l for l in text.splitlines() if l.startswith("[ Early Stop Check")][0].split("now")[1])
    assert abs(now - (met["r_filter_reci_rank"] + met["l_filter_reci_rank"]) / 2) < 1e-9
    assert os.path.exists(os.path.join(out, "stop.txt"))


def test_help_points_to_the_cost_options(capsys):
    with pytest.raises(SystemExit):
        dt.parse_args(["--early_stop_metric", "auc"])
    with pytest.raises(SystemExit):
        dt.parse_args(["--help"])
    helptext = " ".join(capsys.readouterr().out.split())
    # each option: the usage line, its own entry, and the mention in --early_stop_metric's help
    assert helptext.count("--early_stop_rank_triples") >= 3 and helptext.count("--early_stop_stopping_step") >= 3
