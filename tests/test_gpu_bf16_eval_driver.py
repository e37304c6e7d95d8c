"""Training driver on bf16 tables with early stop on validation MRR against drawn candidates: the check ranks from the stored bf16
rows (no float32 view is made at any check), and the logged metric is the one an fp32 Config gives on the checkpoint's tables."""
import os

import pytest

from conftest import GOLDEN
from openkeonspark_amd import distribute_training as dt
from openkeonspark_amd import rank_eval

pytestmark = pytest.mark.gpu

COMMON = ["--input_path", os.path.join(GOLDEN, "kg_small"), "--embedding_dimension", "16", "--n_mini_batches", "2", "--alpha", "0.0",
          "--optimizer", "SGD"]


def test_early_stop_on_mrr_from_the_bf16_tables(tmp_path, capsys, monkeypatch):
    views = []
    real = rank_eval.rank_candidates_device

    def spy(con, dev, tail, head, n_cand, flags, seed, first=0, into=None):
        out = real(con, dev, tail, head, n_cand, flags, seed, first, into)
        views.append((con._bf16, con._eval_view is None, n_cand))
        return out
    monkeypatch.setattr(rank_eval, "rank_candidates_device", spy)
    out = str(tmp_path / "bf16")
    args = dt.parse_args(COMMON + ["--output_path", out, "--train_times", "40", "--early_stop_patience", "2", "--debug", "1",
                                   "--table_dtype", "bf16", "--table_rounding_seed", "5", "--early_stop_metric", "mrr",
                                   "--early_stop_candidates", "16"])
    con = dt.main_fun(args)
    text = capsys.readouterr().out           # lr = 0: the metric cannot improve -> stops after `patience` checks
    assert "Early Stop Check (mrr)" in text and "mrr early stop" in text
    assert con._bf16 and con._tables[0].element_size() == 2
    assert views == [(True, True, 16)] * 3          # three checks, each on the bf16 tables, none with a view
    now = [float(l.split("now")[1]) for l in text.splitlines() if l.startswith("[ Early Stop Check")]
    assert len(now) == 3 and 0.0 < now[-1] <= 1.0
    # an fp32 Config loaded from the run's last checkpoint ranks the same candidates to the same metric
    monkeypatch.setattr(rank_eval, "rank_candidates_device", real)
    last = dt.get_last_step(out)
    assert last == con.global_step
    fp32 = dt.get_conf(dt.parse_args(COMMON))
    fp32.device = con.device
    fp32.set_model_and_session(fp32.model)
    dt.restore_checkpoint(fp32, os.path.join(out, "model.ckpt-%d.npz" % last))
    assert not fp32._bf16 and fp32._tables[0].element_size() == 4
    fp32.init_link_prediction()
    counts, metrics = fp32.validation_link_prediction(test_head=bool(args.test_head), candidates=16, seed=args.early_stop_candidates_seed)
    sides = ("r", "l") if args.test_head else ("r",)
    want = sum(metrics[s + "_filter_reci_rank"] for s in sides) / len(sides)
    # `now` is parsed from the log's "%.10f": equal up to the printed digits, as test_gpu_rank_candidates_driver.py compares.  The
    # rate is 0, so the tables are the rounded initial draw throughout; test_gpu_bf16_eval_config.py covers trained tables.
    assert counts[:, 0, 0].any() and abs(now[-1] - want) < 1e-9, (now, want)
