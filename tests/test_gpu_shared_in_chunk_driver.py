"""distribute_training --shared_negatives_in_chunk K with --shared_negatives_chunk P --shared_negatives_by_relation 1 on a small
synthetic typed graph (TransE, Adagrad, typed candidates): an epoch writes a checkpoint whose shared-negatives record has the fifth
field; a second run of the same command resumes it at that step and trains on, on lists N + K wide; the same checkpoint without
the flag, or with another K, is refused and the refusal names the flag.  That a resumed run repeats the uninterrupted one bit for
bit is tested on the Config (tests/test_gpu_shared_in_chunk_step.py, with the driver's own save_checkpoint / restore_checkpoint)."""
import os

import numpy as np
import pytest

from openkeonspark_amd import distribute_training as dt

pytestmark = pytest.mark.gpu

CHUNK, SEED, BATCHES, NEG, K = 5, 77, 7, 3, 4
TABLES = ("ent_embeddings", "rel_embeddings")


def run(data, out, train_times, in_chunk=K):
    args = ["--input_path", data, "--output_path", out, "--model", "TransE", "--embedding_dimension", "32", "--n_mini_batches", str(BATCHES),
            "--ent_neg_rate", str(NEG), "--alpha", "0.05", "--optimizer", "Adagrad", "--bern_flag", "1", "--train_times", str(train_times),
            "--work_threads", "4", "--shared_negatives_chunk", str(CHUNK), "--shared_negatives_seed", str(SEED),
            "--shared_negatives_by_relation", "1", "--type_constrained_sampling", "1"]
    if in_chunk is not None:
        args += ["--shared_negatives_in_chunk", str(in_chunk)]
    con = dt.main_fun(dt.parse_args(args))
    return con, {k: v.copy() for k, v in con.get_parameters().items()}


def test_the_driver_trains_checkpoints_and_resumes(tmp_path):
    import openkeonspark_amd as ok
    from openkeonspark_amd import synthetic
    data = synthetic.make_typed_dataset(str(tmp_path / "kg503"), synthetic.SMALL_TYPED, entities=503, train=3000, valid=60, test=40)
    out = str(tmp_path / "run")
    con, first = run(data, out, 1)
    assert (con._shared_chunk, con._shared_by_relation, con._shared_in_chunk, con.negative_ent) == (CHUNK, True, K, NEG)
    assert con.sparse_rows and con._adagrad and con.type_constrained_sampling and con.global_step == BATCHES
    cand, pair, perm, chunks = con.shared_negatives_of(BATCHES - 1)
    assert cand.shape[1] == pair.shape[1] == NEG + K
    assert (cand[chunks[:, 1] >= K][:, NEG:] >= 0).all() and (cand[chunks[:, 1] < K][:, -1] == -1).all() and (chunks[:, 1] < K).any()
    z = np.load(os.path.join(out, "model.ckpt-%d.npz" % BATCHES))
    assert [int(x) for x in z["shared_negatives"]] == [CHUNK, SEED, 1, 1, K] and all(k in z.files for k in TABLES)
    con2, resumed = run(data, out, 1)
    assert con2.global_step == 2 * BATCHES and os.path.exists(os.path.join(out, "model.ckpt-%d.npz" % (2 * BATCHES)))
    for k in TABLES:
        assert np.isfinite(resumed[k]).all() and not np.array_equal(resumed[k], first[k]), k          # the resumed run trained on
        assert np.array_equal(z[k], first[k]), k          # ... and the checkpoint holds what the first one left
    # a resume without the flag, or with another K, is refused before anything is restored
    for other in (None, 0, K + 1):
        with pytest.raises(ok.KgeError, match="--shared_negatives_in_chunk") as exc:
            run(data, out, 1, in_chunk=other)
        assert "%d in-chunk candidates" % K in str(exc.value)
