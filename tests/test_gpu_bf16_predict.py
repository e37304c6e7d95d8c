"""kge_predict_bf16 (include/kge_mi355.h, "Evaluation on bf16 tables"): kge_predict's bits on the widened tables, from the stored
bf16 rows.  Widths: both sides of every rung of csrc/team_shape.hpp that a multiple of 8 can reach.  Axis tables tie the kernel to
the fp64 definition without passing through the fp32 kernel (every value is 0 or a power of two, hence a bf16 value, and the score
is an integer no summation order can change); random tables rounded to bf16 must give kge_predict's bits and lie within 1e-5 of
fp64; then the clip branch of l2_normalize, the ends of the launch and the refusals."""
import functools

import numpy as np
import pytest

import bf16_eval_rig as rig
import bf16_ref as ref
import score_ref
from score_ref import exact_scores, exact_tables, random_tables, scores, seed_of

pytestmark = pytest.mark.gpu

RTOL = 1e-5
R = 3
WIDTHS = [8, 16, 24, 32, 40, 64, 72, 128, 136, 256, 264, 512, 520, 1024]
GRID_CAP = 8192          # dispatch_predict's: blocks of 256 threads, 256 / L teams each


def entities_of(D):
    return max(D, 64) + 2


@functools.lru_cache(maxsize=None)
def axis_case(D):
    E = entities_of(D)
    params = exact_tables("transe", E, R, D, D)
    for x in params.values():
        assert np.array_equal(ref.widen(ref.to_bf16(x)).view(np.uint32), x.view(np.uint32))       # every value is a bf16 value
    return params, rig.Tables(params["ent_embeddings"], params["rel_embeddings"])


def pair_ids(E):
    """The first 170 entities (every special axis of score_ref.entity_axes is among them) and the last 40."""
    return np.unique(np.concatenate([np.arange(min(E, 170)), np.arange(max(0, E - 40), E)]))


@pytest.mark.parametrize("D", WIDTHS)
def test_axis_tables_bit_for_bit(D):
    params, tabs = axis_case(D)
    ids = pair_ids(tabs.E)
    h, t, r = (x.ravel() for x in np.meshgrid(ids, ids, np.arange(R), indexing="ij"))
    rc, got = rig.predict(tabs, h, t, r)
    assert rc == 0
    want = exact_scores("transe", params, h, t, r, D, D, "predict")
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, (len(bad), len(got), [(int(h[i]), int(t[i]), int(r[i]), float(got[i]), float(want[i])) for i in bad[:5]])
    assert len(np.unique(want)) >= 3


@pytest.mark.parametrize("scale", [1.0, 1e-3])
@pytest.mark.parametrize("D", WIDTHS)
def test_random_tables_have_kge_predicts_bits_and_lie_within_1e5_of_fp64(D, scale):
    E, n = entities_of(D), 600
    rng = np.random.default_rng(seed_of("bf16-predict-random", D, scale))
    p = random_tables("transe", E, R, D, D, seed_of("bf16-predict-tables", D), scale)
    tabs = rig.Tables.rounded(p["ent_embeddings"], p["rel_embeddings"])
    h, t, r = rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)
    rc, got = rig.predict(tabs, h, t, r)
    rc32, fp32 = rig.predict(tabs, h, t, r, bf16=False)
    assert rc == 0 and rc32 == 0
    bad = np.nonzero(got.view(np.uint32) != fp32.view(np.uint32))[0]
    assert len(bad) == 0, (len(bad), [(float(got[i]), float(fp32[i])) for i in bad[:5]])
    want = scores("transe", {"ent_embeddings": tabs.ent32, "rel_embeddings": tabs.rel32}, h, t, r, D, D, "predict")
    err = np.abs(got.astype(np.float64) - want) / want
    print("D=%d scale=%g worst relative error against fp64 %.3g (bound %g)" % (D, scale, float(err.max()), RTOL))
    assert (want > 0).all() and (err <= RTOL).all(), float(err.max())


@pytest.mark.parametrize("D", rig.MULTIPLE_OF_8_PER_RUNG)
def test_clip_branch_of_l2_normalize(D):
    """All-zero entity rows, an all-zero relation row and rows of elements near 1e-8 (sum of squares below 1e-12): scaled by
    rsqrt(1e-12), not normalised."""
    E = entities_of(D)
    rng = np.random.default_rng(seed_of("bf16-clip", D))
    p = random_tables("transe", E, R, D, D, seed_of("bf16-clip-tables", D), 3.0)
    tiny = lambda shape: (rng.uniform(0.5e-8, 1.5e-8, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    ent, rel = p["ent_embeddings"], p["rel_embeddings"]
    ent[0:2] = 0.0; ent[2:6] = tiny((4, D))
    rel[0] = 0.0; rel[1] = tiny(D)
    tabs = rig.Tables.rounded(ent, rel)
    assert ((tabs.ent32[2:6].astype(np.float64) ** 2).sum(1) < 1e-12).all() and (tabs.ent32[2:6] != 0).all()
    assert ((tabs.rel32[1].astype(np.float64) ** 2).sum() < 1e-12) and (tabs.rel32[1] != 0).all()
    ids = np.concatenate([np.arange(8), rng.integers(8, E, 12)])
    h, t, r = (x.ravel() for x in np.meshgrid(ids, ids, np.arange(R), indexing="ij"))
    rc, got = rig.predict(tabs, h, t, r)
    rc32, fp32 = rig.predict(tabs, h, t, r, bf16=False)
    assert rc == 0 and rc32 == 0 and rig.same_bits(got, fp32)
    want = scores("transe", {"ent_embeddings": tabs.ent32, "rel_embeddings": tabs.rel32}, h, t, r, D, D, "predict")
    # exactly 0 where everything cancels (zero rows on every side, or h == t under the zero relation row); there the kernel may
    # leave the rounding of one product, at most 2^-25 per element, averaged over the row (test_gpu_predict_definition.py)
    zero = want == 0
    assert (zero == ((r == 0) & ((h == t) | ((h < 2) & (t < 2))))).all()
    assert (got[(h < 2) & (t < 2) & (r == 0)] == 0).all()
    assert (got[zero] <= 2.0 ** -25).all(), float(got[zero].max())
    assert (np.abs(got - want)[~zero] <= RTOL * want[~zero]).all(), float((np.abs(got - want)[~zero] / want[~zero]).max())


def length_edges(D):
    L, _ = score_ref.rung_of(D)
    teams = 256 // L
    return [1, teams - 1, teams + 1] + ([GRID_CAP * teams + 1] if D == 16 else [])


@pytest.mark.parametrize("D", rig.MULTIPLE_OF_8_PER_RUNG)
def test_length_edges(D):
    """n = 0 (nothing written), n = 1, one team short of a workgroup, one more than a workgroup, and -- at width 16, where a
    workgroup holds 16 teams -- one triple past the grid cap: the grid-stride loop's second trip.  Ids 0 and E - 1 at both ends."""
    params, tabs = axis_case(D)
    rng = np.random.default_rng(seed_of("bf16-edges", D))
    rc, out = rig.predict(tabs, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert rc == 0 and (out == rig.FILL).all()
    for n in length_edges(D):
        h, t, r = rng.integers(0, tabs.E, n), rng.integers(0, tabs.E, n), rng.integers(0, R, n)
        h[0], t[0], h[-1], t[-1] = 0, tabs.E - 1, tabs.E - 1, 0
        if n > 1:
            r[0], r[-1] = 2, 1
        rc, got = rig.predict(tabs, h, t, r)
        want = exact_scores("transe", params, h, t, r, D, D, "predict")
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert rc == 0 and len(bad) == 0, (n, rc, len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_refusals_leave_the_output_alone():
    params, tabs = axis_case(16)
    h, t, r = np.arange(5), np.arange(5) + 1, np.arange(5) % R
    untouched = lambda out: bool((out == rig.FILL).all())
    for d in (rig.desc(tabs.E, R, 12), rig.desc(tabs.E, R, 1032), rig.desc(tabs.E, R, 16, model=1), rig.desc(tabs.E, R, 16, 8)):
        rc, out = rig.predict(tabs, h, t, r, d=d)          # (refused before a row is read: the tables' real width does not matter)
        assert rc == rig.KGE_ERR_UNSUPPORTED and untouched(out), (d.model, d.ent_dim, d.rel_dim, rc)
    for kw in (dict(ent=None), dict(rel=None)):
        rc, out = rig.predict(tabs, h, t, r, **kw)
        assert rc == rig.KGE_ERR_BAD_ARG and untouched(out), kw
    rc, out = rig.predict(tabs, h, t, r)
    assert rc == 0 and not untouched(out)
