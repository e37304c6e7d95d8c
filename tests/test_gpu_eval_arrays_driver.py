"""Training driver: --derive_type_constraints 1 on a dataset directory without type_constrain.txt derives the type lists from the
triples, writes the file, and the accuracy early stop, --mode test's typed columns and typed sampling run as with the file;
without the flag such a directory behaves as before."""
import os
import shutil

import pytest

from conftest import GOLDEN
from eval_arrays_cases import file_config, n_n_lists, read_kg, snapshot, type_slices
from openkeonspark_amd import distribute_training as dt

pytestmark = pytest.mark.gpu


@pytest.fixture
def no_type_file(tmp_path):
    d = str(tmp_path / "kg")
    os.makedirs(d)
    src = os.path.join(GOLDEN, "kg_small")
    for f in os.listdir(src):
        if f != "type_constrain.txt":
            shutil.copy(os.path.join(src, f), d)
    return d


def run(tmp_path, d, name, extra):
    out = str(tmp_path / name)
    args = dt.parse_args(["--input_path", d, "--output_path", out, "--embedding_dimension", "16", "--n_mini_batches", "2",
                          "--alpha", "0.0", "--train_times", "40", "--early_stop_patience", "2", "--debug", "1"] + extra)
    return out, dt.main_fun(args)


def test_without_the_flag_a_missing_file_means_no_accuracy_check(tmp_path, no_type_file, capsys):
    assert dt.parse_args([]).derive_type_constraints == 0
    out, con = run(tmp_path, no_type_file, "off", ["--train_times", "3"])
    text = capsys.readouterr().out
    assert "Early Stop Check" not in text and not os.path.exists(os.path.join(no_type_file, "type_constrain.txt"))
    metrics = run(tmp_path, no_type_file, "off", ["--mode", "test"])[1]
    # no lists: no candidate is typed, every typed count is zero, so the typed mean ranks are exactly 1
    assert metrics["r_rank_constrain"] == 1.0 == metrics["r_filter_rank_constrain"] and metrics["r_rank"] > 1.0


def test_derived_lists_drive_the_accuracy_early_stop_and_the_typed_columns(tmp_path, no_type_file, capsys):
    out, con = run(tmp_path, no_type_file, "on", ["--derive_type_constraints", "1", "--type_constrained_sampling", "1"])
    text = capsys.readouterr().out
    checks = [l for l in text.splitlines() if l.startswith("[ Early Stop Check (Accuracy)")]
    assert len(checks) == 3 and 0.0 < float(checks[0].split("now")[1]) <= 1.0      # lr = 0: a first value, then `patience` checks
    assert con.lib.kge_typed_sampling() == 1 and con.global_step == 3 * con.nbatches
    con.set_type_constrained_sampling(False)
    # the file was written and reads back as the lists n_n() generates
    assert os.path.exists(os.path.join(no_type_file, "type_constrain.txt"))
    kg = read_kg("kg_small")
    assert type_slices(snapshot(file_config(no_type_file).lib)) == n_n_lists(kg["R"], kg["train"], kg["valid"], kg["test"])
    os.remove(os.path.join(no_type_file, "type_constrain.txt"))
    metrics = run(tmp_path, no_type_file, "on", ["--mode", "test", "--derive_type_constraints", "1"])[1]
    assert metrics["r_rank_constrain"] > 1.0 and metrics["r_filter_rank_constrain"] > 1.0      # typed counts that are not all zero
    assert os.path.exists(os.path.join(no_type_file, "type_constrain.txt"))
