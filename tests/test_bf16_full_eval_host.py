"""The host side of the full-entity evaluators on stored bf16 tables (include/kge_mi355.h, "Evaluation on bf16 tables"), without a
device: kge_rank_triples_bf16 and kge_topk_entities_bf16 refuse every descriptor outside kge_bf16_eval_supported before they look
for a device, Config.set_bf16_evaluation takes two modes, and kge_workspace_bytes counts nothing in a process that allocated
nothing."""
import ctypes
import os
import subprocess
import sys

import pytest

from openkeonspark_amd import _lib

E, R = 1000, 7
KGE_ERR_UNSUPPORTED = -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTSIDE = {"TransH": (_lib.TRANSH, 64, 64), "ent_dim != rel_dim": (_lib.TRANSE, 64, 32), "D % 8 != 0": (_lib.TRANSE, 12, 12),
           "D > 1024": (_lib.TRANSE, 1032, 1032)}


def buffers():
    """Host arrays standing in for device arrays: the refusal comes before anything is read through them."""
    buf = (ctypes.c_int64 * 64)()
    return ctypes.addressof(buf), buf


@pytest.mark.parametrize("name", sorted(OUTSIDE))
def test_rank_triples_bf16_refuses_without_a_device(name):
    L = _lib.lib()
    model, De, Dr = OUTSIDE[name]
    p, keep = buffers()
    L.kge_clear_error()
    rc = L.kge_rank_triples_bf16(ctypes.byref(_lib.ModelDesc(model, 0, E, R, De, Dr, 1.0, 0)), p, p, p, p, p, 4, 1, p, None)
    assert rc == KGE_ERR_UNSUPPORTED and _lib.last_error(L).startswith("kge_rank_triples_bf16: "), _lib.last_error(L)
    assert not any(keep)
    L.kge_clear_error()


@pytest.mark.parametrize("name", sorted(OUTSIDE))
def test_topk_entities_bf16_refuses_without_a_device(name):
    L = _lib.lib()
    model, De, Dr = OUTSIDE[name]
    p, keep = buffers()
    L.kge_clear_error()
    rc = L.kge_topk_entities_bf16(ctypes.byref(_lib.ModelDesc(model, 0, E, R, De, Dr, 1.0, 0)), p, p, p, p, p, 4, 3, 0, p, p, None)
    assert rc == KGE_ERR_UNSUPPORTED and _lib.last_error(L).startswith("kge_topk_entities_bf16: "), _lib.last_error(L)
    assert not any(keep)
    L.kge_clear_error()


def test_set_bf16_evaluation_takes_view_and_stored_only():
    import openkeonspark_amd as pkg
    con = pkg.Config()
    assert con._bf16_evaluation == "view"
    con.set_bf16_evaluation("stored")
    assert con._bf16_evaluation == "stored"
    con.set_bf16_evaluation("view")
    for bad in ("fp32", "", None, 1, "STORED"):
        with pytest.raises(pkg.KgeError):
            con.set_bf16_evaluation(bad)
    assert con._bf16_evaluation == "view"


def test_workspace_bytes_are_zero_in_a_process_that_allocated_nothing():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import ctypes\n"
            "from openkeonspark_amd import _lib\n"
            "L = _lib.lib()\n"
            "live, peak = ctypes.c_int64(-1), ctypes.c_int64(-1)\n"
            "assert L.kge_workspace_bytes(ctypes.byref(live), ctypes.byref(peak), 1) == 0\n"
            "assert L.kge_workspace_bytes(None, None, 0) == 0\n"
            "print(live.value, peak.value)\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["0", "0"]
