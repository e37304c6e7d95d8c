"""distribute_training --model TransR --shared_negatives_chunk P --shared_negatives_by_relation 1 --type_constrained_sampling 1 on a
small synthetic typed graph: an epoch with Adam writes a checkpoint that records [chunk, seed, by_relation, typed] and all three
tables; a second run of the same command resumes it at that step and trains on; the same checkpoint under another chunk, another
seed or untyped candidates is refused, and so are chunks by position.  That a resumed run repeats the lists of the uninterrupted
one is tested on the Config (tests/test_gpu_shared_transr_step.py, with the driver's own save_checkpoint / restore_checkpoint)."""
import os

import numpy as np
import pytest

from openkeonspark_amd import distribute_training as dt

pytestmark = pytest.mark.gpu

CHUNK, SEED, BATCHES = 5, 77, 7
TABLES = ("ent_embeddings", "rel_embeddings", "transfer_matrix")


def run(data, out, train_times, extra=()):
    args = ["--input_path", data, "--output_path", out, "--model", "TransR", "--embedding_dimension", "32", "--n_mini_batches", str(BATCHES),
            "--ent_neg_rate", "3", "--alpha", "0.05", "--optimizer", "Adam", "--bern_flag", "1", "--train_times", str(train_times),
            "--work_threads", "4", "--shared_negatives_chunk", str(CHUNK), "--shared_negatives_seed", str(SEED),
            "--shared_negatives_by_relation", "1", "--type_constrained_sampling", "1"] + list(extra)
    con = dt.main_fun(dt.parse_args(args))
    return con, {k: v.copy() for k, v in con.get_parameters().items()}


def test_the_help_text_names_transr(capsys):
    with pytest.raises(SystemExit):
        dt.parse_args(["--help"])
    assert "With --model TransR (rel_dim up to 512; SGD, Adagrad or Adam)" in " ".join(capsys.readouterr().out.split())


def test_the_driver_trains_checkpoints_and_resumes(tmp_path):
    import openkeonspark_amd as ok
    from openkeonspark_amd import _lib, synthetic
    data = synthetic.make_typed_dataset(str(tmp_path / "kg503"), synthetic.SMALL_TYPED, entities=503, train=3000, valid=60, test=40)
    con, first = run(data, str(tmp_path / "split"), 1)
    assert con.trainModel.model_id == _lib.TRANSR and con._shared_chunk == CHUNK and con._shared_by_relation and con._adam
    assert not con.sparse_inplace and not con.sparse_rows and con.type_constrained_sampling and con.global_step == BATCHES
    assert "chunks" in con._sparse_buf and len(con.shared_negatives_of(BATCHES - 1)) == 4
    z = np.load(str(tmp_path / "split" / ("model.ckpt-%d.npz" % BATCHES)))
    assert [int(x) for x in z["shared_negatives"]] == [CHUNK, SEED, 1, 1] and all(k in z.files for k in TABLES)
    con2, resumed = run(data, str(tmp_path / "split"), 1)
    assert con2.global_step == 2 * BATCHES and os.path.exists(str(tmp_path / "split" / ("model.ckpt-%d.npz" % (2 * BATCHES))))
    for k in TABLES:
        assert np.isfinite(resumed[k]).all() and not np.array_equal(resumed[k], first[k]), k          # the resumed run trained on
        assert np.array_equal(z[k], first[k]), k          # ... and the checkpoint holds what the first one left
    # another chunk, another seed or untyped candidates: another run, refused by the checkpoint's record
    for extra in (["--shared_negatives_chunk", str(CHUNK + 1)], ["--shared_negatives_seed", str(SEED + 1)], ["--type_constrained_sampling", "0"]):
        with pytest.raises(ok.KgeError, match="shared negatives"):
            run(data, str(tmp_path / "split"), 1, extra)
    # chunks by position: TransR has no such step, and says so before anything is restored
    with pytest.raises(ok.KgeError, match="by_relation"):
        run(data, str(tmp_path / "split"), 1, ["--shared_negatives_by_relation", "0", "--type_constrained_sampling", "0"])
