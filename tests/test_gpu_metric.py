"""Metric-level parity: MR / Hits@10 (BASELINE.json's metric) of a model TRAINED by the engine against the same model
trained by the CPU oracle from the same initial parameters and the same sampler seeds.

The reference computes the metric with `testHead / testTail` over the test set (distribute_training.py:465-527,
Test.h:31-249) and reduces it in main_spark.py:430-448.  Here:
  * both trainers draw bit-identical batches (checked elsewhere) and start from identical tables; their fp32
    trajectories drift apart by rounding (different summation orders, hinges near their switch point), so the
    PARAMETERS after thousands of steps are not comparable element-wise -- the METRICS must be;
  * the engine-trained and the oracle-trained tables are both ranked by the device ranker (`kge_link_prediction`, itself
    bit-exact against the compiled reference's testHead/testTail fixtures, tests/test_gpu_lp.py), over the WHOLE test set;
  * on a sample of test triples the oracle's own ranker (oracle predict + Test.h restatement) is run on the
    oracle-trained tables and must give the device ranker's 8-vectors;
  * training must improve the metric against the untrained model.
Graphs: typed synthetic KGs (openkeonspark_amd/synthetic.py: learnable structure; the reference ships no data)."""
import numpy as np
import pytest

from conftest import parity_report
from oracle import oracle

pytestmark = pytest.mark.gpu


def train_both(path, dim, nbatches, n, alpha, epochs, threads=8, model="TransE"):
    import openkeonspark_amd as pkg
    con = pkg.Config()
    con.prefetch_sampling = False
    con.set_in_path(path); con.set_work_threads(8); con.set_bern(0); con.set_dimension(dim); con.set_nbatches(nbatches)
    con.set_ent_neg_rate(n); con.set_alpha(alpha); con.set_margin(1.0); con.set_opt_method("SGD")
    con.set_test_link_prediction(True)
    con.init()
    con.set_model_and_session(getattr(pkg, model))
    init = con.get_parameters()
    kg = oracle.KG(path, work_threads=8, bern=0)
    kg.set_stream_states(con.get_stream_states())
    orc = oracle.Model(model.lower(), con.entTotal, con.relTotal, dim, dim, margin=1.0, params=init)
    B = con.batch_size
    _, untrained = con.link_prediction(test_head=True)
    steps = epochs * con.nbatches
    loss_g = loss_o = None
    for _ in range(steps):
        loss_g = con.train_step(sync=False)
        bh, bt, br, _ = kg.sampling(B, n, 0)
        loss_o = orc.sgd_step(bh, bt, br, B, n, alpha, nthreads=threads)
    loss_g = float(loss_g.item())
    assert con.get_stream_states().tolist() == kg.stream_states().tolist()      # the same batches were drawn throughout
    out_g, met_g = con.link_prediction(test_head=True)
    con.set_parameters(orc.params)
    out_o, met_o = con.link_prediction(test_head=True)
    return con, orc, untrained, (out_g, met_g, loss_g), (out_o, met_o, loss_o), steps


KEYS = ("r_filter_rank", "l_filter_rank", "r_filter_tot", "l_filter_tot", "r_rank", "l_rank", "r_tot", "l_tot")


@pytest.mark.parametrize("graph", ["small_typed", "fb15k237_typed"])
def test_trained_model_reaches_the_oracle_trained_metrics(graph, tmp_path):
    from openkeonspark_amd.synthetic import make_typed_dataset, FB15K237_TYPED, SMALL_TYPED
    if graph == "small_typed":
        path = make_typed_dataset(str(tmp_path / "typed_small"), SMALL_TYPED)
        dim, nbatches, n, alpha, epochs, sample = 32, 10, 4, 3.0, 40, 200
    else:   # configs[0]'s shape: FB15k-237 cardinalities, dim 100, the auto batch 2 721 (nbatches 100)
        path = make_typed_dataset(str(tmp_path / "typed_fb"), FB15K237_TYPED)
        dim, nbatches, n, alpha, epochs, sample = 100, 100, 4, 10.0, 20, 150
    con, orc, untrained, (out_g, met_g, loss_g), (out_o, met_o, loss_o), steps = train_both(path, dim, nbatches, n, alpha, epochs)
    # (1) the oracle's own ranker on the oracle-trained tables == the device ranker's 8-vectors (sample of the test set)
    ev = oracle.Eval(path)
    E = con.entTotal
    ar = np.arange(E)
    flips = 0
    for i in range(min(sample, ev.testTotal)):
        h, t, r = ev.test_triple(i)
        for side, fixed_scores, target in ((0, orc.predict(np.full(E, h), ar, np.full(E, r)), t),
                                           (1, orc.predict(ar, np.full(E, t), np.full(E, r)), h)):
            want = ev.rank(i, fixed_scores, head=bool(side))
            got = out_o[i, side]
            if got[:4].tolist() != want[:4].tolist():
                # the two rankers count candidates scoring STRICTLY below the target (Test.h:60,170) on fp32 scores from two
                # implementations (sums over the dimension in different orders): a differing count must come from a candidate whose
                # score is within 2e-6 relative of the target's
                # (several candidates can sit at such a near-tie at once -- seen: two, 1.5e-8 from the target -- so the counts may
                # differ by as many as there are candidates inside that band, not just by one)
                flips += 1
                others = np.abs(np.delete(fixed_scores, target) - fixed_scores[target])
                near = int((others <= 2e-6 * abs(fixed_scores[target])).sum())
                assert 1 <= np.abs(got[:4] - want[:4]).max() <= near, (i, side, got, want, near, others.min())
    # (2) metric-level agreement of the two trainers, whole test set, both sides
    report = dict(graph=graph, steps=steps, test_triples=int(ev.testTotal), final_loss_engine=loss_g, final_loss_oracle=loss_o,
                  ranker_vectors_differing_by_one=flips, ranker_vectors_checked=2 * min(sample, ev.testTotal))
    for k in KEYS:
        report[k] = dict(untrained=untrained[k], engine=met_g[k], oracle=met_o[k])
    parity_report("metric_parity[%s]" % graph, **report)
    assert flips <= 0.03 * report["ranker_vectors_checked"], flips   # each one explained above: a near-tie of two scores
    for side in ("r", "l"):
        mr_g, mr_o, mr_0 = met_g[side + "_filter_rank"], met_o[side + "_filter_rank"], untrained[side + "_filter_rank"]
        h10_g, h10_o, h10_0 = met_g[side + "_filter_tot"], met_o[side + "_filter_tot"], untrained[side + "_filter_tot"]
        # filtered MR within 5 %, or 2.5 standard errors of the mean rank on a test set this small (the two trainers' fp32
        # trajectories differ by the order of their atomic adds: on 400 test triples that alone moves MR by several per cent)
        ranks = 1.0 + out_g[:, 0 if side == "r" else 1, 1]
        mr_tol = max(0.05 * mr_o, 2.5 * float(ranks.std()) / np.sqrt(len(ranks)))
        assert abs(mr_g - mr_o) <= mr_tol, (side, mr_g, mr_o, mr_tol)
        # filtered Hits@10 within 0.02 absolute, or 2.5 binomial standard deviations of a test set this small (400 triples: 0.05)
        h10_tol = max(0.02, 2.5 * np.sqrt(max(h10_o * (1 - h10_o), 0.05) / ev.testTotal))
        assert abs(h10_g - h10_o) <= h10_tol, (side, h10_g, h10_o, h10_tol)
        assert mr_g < 0.75 * mr_0 and mr_o < 0.75 * mr_0, (side, mr_g, mr_o, mr_0)  # training helps: MR falls by > 25 %
        assert h10_g > h10_0 and h10_o > h10_0
    assert abs(loss_g - loss_o) <= 0.15 * max(loss_o, 1e-3) + 0.01


@pytest.mark.parametrize("model", ["TransH", "TransD"])
def test_trained_through_the_pair_count_path_reaches_the_oracle_trained_metrics(model, tmp_path):
    """The same comparison for TransH / TransD with 8 negatives per positive, every step through the pair-count path (csrc/pairs.hip:
    int8 sign records keyed by (entity, relation), backward once per pair; forced here for this small graph): engine-trained
    and oracle-trained tables ranked by the device ranker over the whole test set."""
    from openkeonspark_amd import _lib
    from openkeonspark_amd.synthetic import make_typed_dataset, SMALL_TYPED
    path = make_typed_dataset(str(tmp_path / "typed_small"), SMALL_TYPED)
    L = _lib.lib()
    L.kge_set_option(b"float_records_min", 0)
    try:
        con, orc, untrained, (out_g, met_g, loss_g), (out_o, met_o, loss_o), steps = train_both(path, 32, 10, 8, 3.0, 30, model=model)
        assert L.kge_pair_path_active(__import__("ctypes").byref(con._desc), con.batch_size, 8) == 1
    finally:
        L.kge_set_option(b"float_records_min", 1 << 16)
    report = dict(graph="small_typed", model=model, negatives=8, steps=steps, final_loss_engine=loss_g, final_loss_oracle=loss_o)
    for k in KEYS:
        report[k] = dict(untrained=untrained[k], engine=met_g[k], oracle=met_o[k])
    parity_report("metric_parity[%s-pair-count-path]" % model.lower(), **report)
    n_test = out_g.shape[0]
    for side in ("r", "l"):
        mr_g, mr_o, mr_0 = met_g[side + "_filter_rank"], met_o[side + "_filter_rank"], untrained[side + "_filter_rank"]
        h10_g, h10_o = met_g[side + "_filter_tot"], met_o[side + "_filter_tot"]
        ranks = 1.0 + out_g[:, 0 if side == "r" else 1, 1]
        mr_tol = max(0.05 * mr_o, 2.5 * float(ranks.std()) / np.sqrt(len(ranks)))
        assert abs(mr_g - mr_o) <= mr_tol, (side, mr_g, mr_o, mr_tol)
        h10_tol = max(0.02, 2.5 * np.sqrt(max(h10_o * (1 - h10_o), 0.05) / n_test))
        assert abs(h10_g - h10_o) <= h10_tol, (side, h10_g, h10_o, h10_tol)
        assert mr_g < 0.9 * mr_0 and mr_o < 0.9 * mr_0, (side, mr_g, mr_o, mr_0)   # training helps
    assert abs(loss_g - loss_o) <= 0.15 * max(loss_o, 1e-3) + 0.01
