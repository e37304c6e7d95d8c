"""kge_bf16_eval_supported (include/kge_mi355.h, "Evaluation on bf16 tables"): a host-only query that needs no device.  1 exactly
for TransE with ent_dim == rel_dim, D % 8 == 0 and 8 <= D <= 1024 -- the storage rule of "bf16 table storage"."""
import ctypes

import pytest

from openkeonspark_amd import _lib

E, R = 1000, 7


def supported(model, De, Dr):
    return _lib.lib().kge_bf16_eval_supported(ctypes.byref(_lib.ModelDesc(model, 0, E, R, De, Dr, 1.0, 0)))


@pytest.mark.parametrize("D", [8, 200, 1024])
def test_transe_widths_inside_the_rule(D):
    assert supported(_lib.TRANSE, D, D) == 1


@pytest.mark.parametrize("D", [4, 12, 1032])
def test_transe_widths_outside_the_rule(D):
    assert supported(_lib.TRANSE, D, D) == 0


def test_entity_and_relation_widths_must_agree():
    assert supported(_lib.TRANSE, 64, 32) == 0 and supported(_lib.TRANSE, 32, 64) == 0


@pytest.mark.parametrize("model", [_lib.TRANSH, _lib.TRANSD, _lib.TRANSR])
def test_other_models_are_refused(model):
    assert supported(model, 64, 64) == 0


def test_the_rule_does_not_depend_on_the_table_sizes():
    """Unlike kge_bf16_tables_supported there is no row limit and no negative count: a table of 2^30 rows that cannot be trained
    in this mode can still be scored."""
    L = _lib.lib()
    big = _lib.ModelDesc(_lib.TRANSE, 0, 1 << 30, R, 64, 64, 1.0, 0)
    assert L.kge_bf16_eval_supported(ctypes.byref(big)) == 1 and L.kge_bf16_tables_supported(ctypes.byref(big), 1) == 0
    assert L.kge_bf16_eval_supported(None) == 0
