"""Training driver on bf16 tables with --bf16_evaluation stored and early stop on the exact validation MRR (every entity a
candidate): the check ranks from the stored bf16 rows (no float32 view exists at any check), and the logged metric is the one an
fp32 Config gives on the checkpoint's tables."""
import os

import pytest

from conftest import GOLDEN
from openkeonspark_amd import distribute_training as dt
from openkeonspark_amd import rank_eval

pytestmark = pytest.mark.gpu

COMMON = ["--input_path", os.path.join(GOLDEN, "kg_small"), "--embedding_dimension", "16", "--n_mini_batches", "2", "--alpha", "0.0",
          "--optimizer", "SGD"]


def test_early_stop_on_exact_mrr_from_the_stored_bf16_tables(tmp_path, capsys, monkeypatch):
    checks = []
    real = rank_eval.rank_device

    def spy(con, dev, test_head, into=None):
        before = con._eval_view is None
        out = real(con, dev, test_head, into)
        checks.append((con._bf16, con._bf16_evaluation, before, con._eval_view is None))
        return out
    monkeypatch.setattr(rank_eval, "rank_device", spy)
    out = str(tmp_path / "bf16")
    args = dt.parse_args(COMMON + ["--output_path", out, "--train_times", "40", "--early_stop_patience", "2", "--debug", "1",
                                   "--table_dtype", "bf16", "--table_rounding_seed", "5", "--early_stop_metric", "mrr",
                                   "--bf16_evaluation", "stored"])
    assert args.early_stop_candidates == 0
    con = dt.main_fun(args)
    text = capsys.readouterr().out           # lr = 0: the metric cannot improve -> stops after `patience` checks
    assert "Early Stop Check (mrr)" in text and "mrr early stop" in text
    assert con._bf16 and con._tables[0].element_size() == 2
    assert checks == [(True, "stored", True, True)] * 3          # three checks, each on the stored rows, none with a view
    now = [float(l.split("now")[1]) for l in text.splitlines() if l.startswith("[ Early Stop Check")]
    assert len(now) == 3 and 0.0 < now[-1] <= 1.0
    # an fp32 Config loaded from the run's last checkpoint ranks every entity to the same metric
    monkeypatch.setattr(rank_eval, "rank_device", real)
    last = dt.get_last_step(out)
    assert last == con.global_step
    fp32 = dt.get_conf(dt.parse_args(COMMON))
    fp32.device = con.device
    fp32.set_model_and_session(fp32.model)
    dt.restore_checkpoint(fp32, os.path.join(out, "model.ckpt-%d.npz" % last))
    assert not fp32._bf16 and fp32._tables[0].element_size() == 4
    fp32.init_link_prediction()
    counts, metrics = fp32.validation_link_prediction(test_head=bool(args.test_head))
    sides = ("r", "l") if args.test_head else ("r",)
    want = sum(metrics[s + "_filter_reci_rank"] for s in sides) / len(sides)
    # `now` is parsed from the log's "%.10f": equal up to the printed digits.  The rate is 0, so the tables are the rounded
    # initial draw throughout; test_gpu_bf16_full_eval_config.py covers trained tables.
    assert counts[:, 0, 0].any() and abs(now[-1] - want) < 1e-9, (now, want)


def test_the_driver_takes_view_by_default_and_refuses_other_modes():
    assert dt.parse_args(COMMON).bf16_evaluation == "view"
    with pytest.raises(SystemExit):
        dt.parse_args(COMMON + ["--bf16_evaluation", "fp32"])
