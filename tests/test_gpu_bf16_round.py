"""kge_bf16_round_stochastic -- the stochastic rounding rule of bf16 table storage alone -- against its numpy restatement
(tests/bf16_ref.py), bit for bit: special values, values on the bf16 grid, random values; two seeds, two steps, a first key other
than zero; widths with one and with many mixes per row and more than one workgroup."""
import ctypes

import numpy as np
import pytest

import bf16_ref as ref

pytestmark = pytest.mark.gpu


def device_round(y, first_key, seed, step):
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    rows, D = y.shape
    d_y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    out = torch.zeros((rows, D), dtype=torch.int16, device="cuda")
    _lib.check(L.kge_bf16_round_stochastic(d_y.data_ptr(), rows, D, first_key, ctypes.c_uint64(seed), ctypes.c_uint64(step), out.data_ptr(),
                                           None), L)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)


def special_rows(D):
    f = np.float32
    vals = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 2.0 ** -126, 3.4028234663852886e38, -3.4028234663852886e38, np.inf, -np.inf,
                     np.nan, 1.0, -1.5, 3.140625, 2.0 ** -133, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8, -(1.0 + 2.0 ** -23), 0.1], dtype=f)
    rows = -(-4 * len(vals) // D) * 4
    return np.resize(vals, (rows, D)).astype(f)


@pytest.mark.parametrize("D", [8, 200, 1024])
@pytest.mark.parametrize("seed,step,first_key", [(0, 0, 0), (0, 1, 0), (0xDEADBEEFCAFEF00D, 0, 0), (7, 41, 12345), (7, 41, 500 + 3)])
def test_the_hook_equals_the_restatement(D, seed, step, first_key):
    rng = np.random.default_rng(D + step)
    rows = 700 if D == 8 else 300           # more than one workgroup's worth of elements at every width
    y = np.concatenate([special_rows(D),
                        (rng.standard_normal((rows, D)) * 10.0 ** rng.integers(-3, 3, (rows, 1))).astype(np.float32),
                        ref.widen(ref.to_bf16(rng.standard_normal((16, D)).astype(np.float32)))])      # on the bf16 grid
    got = device_round(y, first_key, seed, step)
    want = ref.round_rows(y, first_key + np.arange(y.shape[0]), seed, step)
    np.testing.assert_array_equal(got, want)
    grid = y.shape[0] - 16
    np.testing.assert_array_equal(got[grid:], y[grid:].view(np.uint32) >> 16)      # grid values keep their bits
    assert np.isnan(ref.widen(got)[np.isnan(y)]).all() and np.isinf(ref.widen(got)[np.isinf(y)]).all()


def test_seeds_steps_and_keys_give_other_bits():
    rng = np.random.default_rng(3)
    y = rng.standard_normal((64, 64)).astype(np.float32)
    a = device_round(y, 0, 1, 0)
    assert (a != device_round(y, 0, 2, 0)).mean() > 0.3 and (a != device_round(y, 0, 1, 1)).mean() > 0.3
    assert (a != device_round(y, 64, 1, 0)).mean() > 0.3
    np.testing.assert_array_equal(a[32:], device_round(y[32:], 32, 1, 0))      # the key is first_key + row


def test_bad_arguments_are_refused():
    import torch
    from openkeonspark_amd import _lib
    L = _lib.lib()
    y = torch.zeros((4, 20), device="cuda")
    out = torch.zeros((4, 20), dtype=torch.int16, device="cuda")
    for D in (20, 4, 1032):
        assert L.kge_bf16_round_stochastic(y.data_ptr(), 4, D, 0, 0, 0, out.data_ptr(), None) != 0
    L.kge_clear_error()
