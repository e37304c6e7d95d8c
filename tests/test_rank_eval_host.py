"""The host half of openkeonspark_amd.rank_eval: the split of n items across ranks, the seed shift of drawn candidate lists, the
metric accumulators from hand-made counts, the one argument checker and the import direction Config -> rank_eval -> shard_eval.
No GPU and no engine."""
import inspect
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from openkeonspark_amd import _lib, rank_eval, shard_eval
from openkeonspark_amd._lib import KgeError


def test_the_slices_of_every_rank_cover_the_items_once():
    for W in range(1, 6):
        for n in range(0, 13):
            per = (n + W - 1) // W
            slices = [rank_eval.rank_slice(n, g, W) for g in range(W)]
            assert slices == [(min(g * per, n), min((g + 1) * per, n)) for g in range(W)], (W, n)
            assert slices[0][0] == 0 and slices[-1][1] == n
            assert all(c0 <= c1 for c0, c1 in slices)
            assert all(slices[g][1] == slices[g + 1][0] for g in range(W - 1))          # contiguous, so disjoint
            assert sorted(i for c0, c1 in slices for i in range(c0, c1)) == list(range(n))


@pytest.mark.parametrize("seed", [0, 5, 2 ** 63 + 12345, 2 ** 64 - 1])
@pytest.mark.parametrize("first", [0, 1, 11, 2 ** 31 - 1])
def test_the_shifted_seed_draws_what_the_global_index_draws(seed, first):
    i, k = np.arange(4)[:, None], np.arange(6)[None, :]
    moved = _lib.drawn_seed_at(seed, first)
    assert 0 <= moved < 2 ** 64
    for side in (0, 1):
        for length in (1, 7, 14541):
            assert np.array_equal(_lib.drawn_candidate_index(moved, i, side, k, length),
                                  _lib.drawn_candidate_index(seed, first + i, side, k, length)), (side, length)


def restated(cnt):
    """Hits@k = count < k, MR = 1 + count, MRR = 1 / (1 + count), summed over the triples: (the five name parts, the value)."""
    return {("", "_tot"): float((cnt < 10).sum()), ("3", "_tot"): float((cnt < 3).sum()), ("1", "_tot"): float((cnt < 1).sum()),
            ("", "_rank"): float((1 + cnt).sum()), ("", "_reci_rank"): float((1.0 / (1 + cnt)).sum())}


def want_sums(columns):
    """{name: value} for {(stem, "" or "_filter", "" or "_constrain"): count column}."""
    return {stem + k + name + end + suffix: v for (stem, name, suffix), cnt in columns.items() for (k, end), v in restated(cnt).items()}


KINDS = (("", ""), ("_filter", ""), ("", "_constrain"), ("_filter", "_constrain"))        # columns 0..3


def test_link_prediction_sums_from_hand_made_counts():
    out = np.zeros((4, 2, 8), np.int64)
    out[:, 0, :4] = np.array([[0, 1, 3, 10], [0, 0, 2, 9], [1, 2, 9, 11], [0, 1, 2, 3]]).T
    out[:, 1, :4] = np.array([[10, 3, 1, 0], [9, 2, 0, 0], [100, 10, 3, 1], [2, 2, 2, 2]]).T
    out[:, :, 4:] = 77          # the arg-min columns are not counts and enter no metric
    want = want_sums({(stem, name, suffix): out[:, side, col] for side, stem in ((0, "r"), (1, "l"))
                      for col, (name, suffix) in enumerate(KINDS)})
    got = rank_eval.lp_sums(out)
    assert len(want) == 40 and set(got) == set(want) and got == want
    assert got["r_tot"] == 3.0 and got["r3_tot"] == 2.0 and got["r1_tot"] == 1.0 and got["r_rank"] == 18.0
    tail_only = rank_eval.lp_sums(out, test_head=False)
    assert len(tail_only) == 20 and not any(k.startswith("l") for k in tail_only)
    assert tail_only == {k: v for k, v in want.items() if k.startswith("r")}
    assert rank_eval.normalise(got, 4) == {k: v / 4.0 for k, v in want.items()}
    assert rank_eval.normalise(got, 0) == want          # no triples: divided by 1


def test_candidate_sums_from_hand_made_counts():
    counts = np.zeros((4, 2, 2), np.int64)
    counts[:, 0] = np.array([[0, 2, 9, 10], [0, 0, 3, 9]]).T
    counts[:, 1] = np.array([[1, 1, 3, 100], [0, 1, 1, 50]]).T
    want = want_sums({(stem, name, ""): counts[:, side, col] for side, stem in ((0, "r"), (1, "l"))
                      for col, name in enumerate(("", "_filter"))})
    got = rank_eval.cand_sums(counts)
    assert len(want) == 20 and set(got) == set(want) and got == want
    tail = rank_eval.cand_sums(counts, (0,))
    assert len(tail) == 10 and tail == {k: v for k, v in want.items() if k.startswith("r")}
    assert not any("constrain" in k for k in got)


def test_relation_sums_from_hand_made_counts():
    out = np.array([[0, 0, 0, 0], [1, 0, 1, 0], [3, 2, 3, 1], [10, 9, 12, 10]], np.int64)
    want = want_sums({("rel", name, suffix): out[:, col] for col, (name, suffix) in enumerate(KINDS)})
    got = rank_eval.rel_sums(out)
    assert len(want) == 20 and set(got) == set(want) and got == want
    assert got["rel_tot"] == 3.0 and got["rel_filter_tot"] == 4.0 and got["rel3_tot_constrain"] == 2.0 and got["rel1_filter_tot_constrain"] == 2.0


@pytest.mark.parametrize("kind", [KgeError, ValueError, TypeError, OverflowError, OSError, RuntimeError, AttributeError])
def test_the_checker_keeps_what_the_check_raised(kind):
    def thunk():
        raise kind("bad argument")
    value, err = rank_eval.checked(thunk)
    assert value is None and type(err) is kind and str(err) == "bad argument"


def test_the_checker_returns_the_value_and_lets_other_exceptions_through():
    assert rank_eval.checked(lambda: (1, "a")) == ((1, "a"), None)
    with pytest.raises(KeyError):
        rank_eval.checked(lambda: {}["missing"])


def test_shard_eval_calls_nothing_back():
    src = inspect.getsource(shard_eval)
    assert "con._topk" not in src and "con._rank_device" not in src
    # a fresh interpreter imports the module by its own imports alone: the package's __init__ imports Config (and with it
    # rank_eval) for the public names, so the package is entered as a bare namespace over the same directory
    code = ("import os, sys, types\n"
            "pkg = types.ModuleType('openkeonspark_amd'); pkg.__path__ = [os.path.join(%r, 'openkeonspark_amd')]\n"
            "sys.modules['openkeonspark_amd'] = pkg\n"
            "import openkeonspark_amd.shard_eval as m\n"
            "assert callable(m.agree) and 'openkeonspark_amd._lib' in sys.modules\n"
            "sys.exit(3 if 'openkeonspark_amd.rank_eval' in sys.modules or 'openkeonspark_amd.Config' in sys.modules else 0)\n" % ROOT)
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
