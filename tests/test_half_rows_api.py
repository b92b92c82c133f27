"""CPU: the eligibility rule of the half-precision shadow rows (include/wann.h wann_rows_fp16_exact), through the C ABI.  A
float32 point set may be searched from half rows only if every value is a finite IEEE binary16 value."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib(wa):
    import rangefilteredann_amd
    L = ctypes.CDLL(rangefilteredann_amd.lib_path())
    L.wann_rows_fp16_exact.restype = ctypes.c_int
    L.wann_rows_fp16_exact.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    return L


def _exact(lib, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    return lib.wann_rows_fp16_exact(a.ctypes.data, a.shape[0], a.shape[1])


def test_binary16_values_are_accepted(lib):
    assert _exact(lib, np.arange(0, 2049)) == 1  # (every integer up to 2^11 is a binary16 value)
    assert _exact(lib, -np.arange(0, 2049)) == 1
    for v in (65504.0, -65504.0, -0.0, 2.0 ** -24, 2.0 ** -14, -(2.0 ** -24), 1023 * 2.0 ** -24, 0.5, 1 + 2.0 ** -10):
        assert _exact(lib, [v]) == 1, v
    # the test is on bits, not on values: -0.0 is kept as -0.0
    assert np.float32(-0.0).view(np.uint32) == 0x80000000


@pytest.mark.parametrize("v", [2049.0, 65520.0, 65505.0, 1 + 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 0.1, 1e30, float("nan"),
                               float("inf"), -float("inf")])
def test_other_values_are_refused(lib, v):
    assert _exact(lib, [v]) == 0
    assert _exact(lib, [1.0, v, 2.0]) == 0


def test_every_nan_is_refused(lib):
    # the default NaN and the infinities survive float -> half -> float bit for bit: they are refused by their exponent
    for bits in (0x7FC00000, 0xFFC00000, 0x7FC02000, 0x7F800001, 0x7F800000, 0xFF800000):
        a = np.array([[bits]], dtype=np.uint32).view(np.float32)
        assert _exact(lib, a) == 0, hex(bits)


def test_one_bad_value_at_the_end_of_a_large_array(lib):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, size=(1000, 20)).astype(np.float32)
    assert _exact(lib, a) == 1
    a[-1, -1] = 0.1
    assert _exact(lib, a) == 0
    a[-1, -1] = 7
    a[0, 0] = 0.1
    assert _exact(lib, a) == 0
    a[0, 0] = 7
    a[500, 3] = 4097
    assert _exact(lib, a) == 0


def test_empty_set_is_exact(lib):
    assert lib.wann_rows_fp16_exact(None, 0, 20) == 1
    a = np.zeros((0, 20), dtype=np.float32)
    assert lib.wann_rows_fp16_exact(a.ctypes.data, 0, 20) == 1


def test_agrees_with_numpy_on_random_bit_patterns(lib):
    rng = np.random.default_rng(6)
    h = rng.integers(0, 1 << 16, size=4096, dtype=np.uint32).astype(np.uint16).view(np.float16)
    for x in h.astype(np.float32):
        assert _exact(lib, [x]) == (1 if np.isfinite(x) else 0)
    f = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        back = f.astype(np.float16).astype(np.float32)
    for x, b in zip(f, back):
        want = 1 if (np.isfinite(x) and x.view(np.uint32) == b.view(np.uint32)) else 0
        assert _exact(lib, [x]) == want, hex(int(x.view(np.uint32)))
