"""The engine's process-global device workspaces (csrc/dev_buf.hpp) across regrowth.  They only grow and earlier tests of a
process have grown them already, so every case runs in child processes of its own (tests/regrow_cases.py): one child makes
call A at a small shape, call B at a larger one and A again -- A must give what it gave before B regrew the buffers under it --
and a second child makes B first, on buffers allocated at B's size from nothing, which must equal the first child's B, made
on buffers regrown from A's.  Integer results, and the paths DESIGN.md documents as reproducible bit for bit (the sign-count
step, LazyAdam on the touched rows), are compared exactly; the others with the tolerance their own tests use, quoted below."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_dev_buf_host import build_and_run
from test_gpu_persistent import update_err

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "regrow_cases.py")


def run(case, order, tmp_path):
    path = str(tmp_path / ("%s_%s.npz" % (case, order)))
    res = subprocess.run([sys.executable, CHILD, case, order, path], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok"), res.stdout[-2000:] + res.stderr[-4000:]
    z = np.load(path)
    calls = [{} for _ in order]
    for key in z.files:
        i, name = key.split("/", 1)
        calls[int(i)][name] = z[key]
    return calls


def exact(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def ids_exact_scores_close(a, b, what):
    """ids and ranks are integers; the scores to tests/test_gpu_topk.py close / tests/test_gpu_relpred.py tol:
    |a - b| <= 1e-6 + 1e-5 |b|"""
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype.kind == "f":
            fin = np.isfinite(b[k])
            assert np.array_equal(fin, np.isfinite(a[k])) and np.array_equal(a[k][~fin], b[k][~fin], equal_nan=True), (what, k)
            assert (np.abs(a[k][fin] - b[k][fin]) <= 1e-6 + 1e-5 * np.abs(b[k][fin])).all(), (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def transr_close(a, b, what):
    """TransR's wgrad adds in fp32 atomics: tests/test_gpu_models.py
    test_transr_sampler_riding_in_the_relation_scatter_draws_the_same_batches holds two runs of the same steps to
    np.allclose(losses, rtol=2e-6, atol=0) and max |p - q| <= 1e-5 max |p| per table, the rng states to equality."""
    assert a["streams"].tolist() == b["streams"].tolist(), what
    assert np.allclose(a["losses"], b["losses"], rtol=2e-6, atol=0), (what, a["losses"], b["losses"])
    for k in a:
        if k.startswith("p/"):
            assert np.abs(a[k] - b[k]).max() <= 1e-5 * np.abs(a[k]).max(), (what, k)


def persistent_close(a, b, what):
    """fp32 atomics in either form: tests/test_gpu_persistent.py test_persistent_steps_equal_separate_launches holds two SGD
    runs of the same steps to equal rng states, np.allclose(losses[:3], rtol=1e-5), np.allclose(losses, rtol=1e-4) and at
    most max(3, 1 %) of the rows with an accumulated update off by more than 2e-5 of the table's largest."""
    assert a["streams"].tolist() == b["streams"].tolist(), what
    assert np.allclose(a["losses"][:3], b["losses"][:3], rtol=1e-5, atol=0), (what, a["losses"], b["losses"])
    assert np.allclose(a["losses"], b["losses"], rtol=1e-4, atol=0), (what, a["losses"], b["losses"])
    start = {k[6:]: v for k, v in a.items() if k.startswith("start/")}
    pa, pb = ({k[2:]: v for k, v in x.items() if k.startswith("p/")} for x in (a, b))
    for k in start:
        assert np.array_equal(start[k], b["start/" + k]), (what, k)
    outside, worst, total = update_err(pa, pb, start, 2e-5)
    print("[regrow] %s: rows outside %d of %d, worst other %.3g" % (what, outside, total, worst))
    assert outside <= max(3, 0.01 * total), (what, outside, total)


@pytest.mark.parametrize("case,same", [
    ("rank_transr", exact),
    ("relpred_transr", ids_exact_scores_close),
    ("topk_tails", ids_exact_scores_close),
    ("link_prediction", exact),
    ("lazy_adam_transh", exact),
    ("transr_groups", transr_close),
    ("transe_counts", exact),
    ("persistent", persistent_close),
])
def test_small_large_small_and_large_first(case, same, tmp_path):
    a0, b, a1 = run(case, "ABA", tmp_path)
    same(a0, a1, case + ": A before and after B")
    (b_first,) = run(case, "B", tmp_path)
    same(b, b_first, case + ": B after A and B first")
    if case == "link_prediction":            # the two routes agree (tests/test_gpu_lp.py), also when `cand` is sized after `scores`
        for x in (a0, b, a1, b_first):
            assert np.array_equal(x["out0"], x["out1"]) and np.array_equal(x["out0"], x["out2"])


def test_dev_buf_contract_with_a_device(tmp_path):
    """tests/dev_buf_host_main.cpp with the device visible: the success half of what test_dev_buf_host.py checks."""
    checks, failed, calls, allocated = build_and_run(tmp_path, hide_devices=False)
    assert failed == 0 and allocated == 2
