"""CPU: the eligibility rule of the one-byte shadow rows (include/wann.h wann_rows_u8_exact), through the C ABI.  A float32
point set may be searched from one-byte rows only if every value is an integer 0 .. 255 with the bits of (float)(uint8_t)x."""
import ctypes
import os

import numpy as np
import pytest

from util import REPO

SYMBOLS = ("wann_rows_u8_exact", "wann_set_byte_rows", "wann_byte_rows", "wann_byte_rows_bytes", "wann_last_byte_rows")


@pytest.fixture(scope="module")
def lib(wa):
    import rangefilteredann_amd
    L = ctypes.CDLL(rangefilteredann_amd.lib_path())
    L.wann_rows_u8_exact.restype = ctypes.c_int
    L.wann_rows_u8_exact.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    return L


def _exact(lib, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    return lib.wann_rows_u8_exact(a.ctypes.data, a.shape[0], a.shape[1])


def _numpy_rule(x):
    """(float)(uint8_t)x has the bits of x, for x in [0, 255] (outside it the conversion to uint8 is not defined)"""
    x = np.float32(x)
    if not (0 <= x <= 255):  # (false for NaN)
        return 0
    back = np.array([x]).astype(np.uint8).astype(np.float32)[0]
    return 1 if back.view(np.uint32) == x.view(np.uint32) else 0


def test_every_uint8_value_is_accepted(lib):
    assert _exact(lib, np.arange(0, 256)) == 1
    for v in range(256):
        assert _exact(lib, [float(v)]) == 1, v


@pytest.mark.parametrize("v", [-0.0, -1.0, 256.0, 0.5, 254.5, 2.0 ** -149, 1e30, float("inf"), -float("inf"), float("nan")])
def test_other_values_are_refused(lib, v):
    assert _exact(lib, [v]) == 0
    assert _exact(lib, [1.0, v, 2.0]) == 0


def test_the_rule_is_on_bits(lib):
    # -0.0 == 0.0 as a value; its bits are not those of (float)(uint8_t)0
    assert np.float32(-0.0).view(np.uint32) == 0x80000000 and np.float32(-0.0) == 0
    a = np.array([[0x80000000]], dtype=np.uint32).view(np.float32)
    assert _exact(lib, a) == 0
    assert _exact(lib, np.array([[0]], dtype=np.uint32).view(np.float32)) == 1


def test_every_nan_is_refused(lib):
    for bits in (0x7FC00000, 0xFFC00000, 0x7FC02000, 0x7F800001, 0x7F800000, 0xFF800000):
        a = np.array([[bits]], dtype=np.uint32).view(np.float32)
        assert _exact(lib, a) == 0, hex(bits)


def test_one_bad_value_at_the_start_middle_and_end_of_a_large_array(lib):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, size=(1000, 20)).astype(np.float32)
    assert _exact(lib, a) == 1
    for at, bad in (((0, 0), 0.5), ((500, 3), 256.0), ((-1, -1), -1.0)):
        was = a[at]
        a[at] = bad
        assert _exact(lib, a) == 0, at
        a[at] = was
    assert _exact(lib, a) == 1


def test_empty_set_is_exact(lib):
    assert lib.wann_rows_u8_exact(None, 0, 20) == 1
    a = np.zeros((0, 20), dtype=np.float32)
    assert lib.wann_rows_u8_exact(a.ctypes.data, 0, 20) == 1


def test_agrees_with_numpy(lib):
    rng = np.random.default_rng(6)
    f = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    for x in f:
        assert _exact(lib, [x]) == _numpy_rule(x), hex(int(x.view(np.uint32)))
    accepted = 0
    for x in np.arange(-300, 300.5, 0.5, dtype=np.float32):
        got = _exact(lib, [x])
        assert got == _numpy_rule(x), x
        accepted += got
    assert accepted == 256


def test_symbols_and_header(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.wann_abi_version() == 5
    header = open(os.path.join(REPO, "include", "wann.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name
    # a null index: no copy, no setting, a negative error for the setter
    lib.wann_byte_rows_bytes.restype = ctypes.c_int64
    lib.wann_set_byte_rows.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for f in (lib.wann_byte_rows, lib.wann_last_byte_rows, lib.wann_byte_rows_bytes):
        f.argtypes = [ctypes.c_void_p]
    assert lib.wann_set_byte_rows(None, 1) < 0
    assert lib.wann_byte_rows(None) == 0 and lib.wann_last_byte_rows(None) == 0 and lib.wann_byte_rows_bytes(None) == -1


def test_six_is_not_a_public_dtype(wa, lib):
    """the internal view type of the one-byte rows is refused by wann_index_create like any unknown dtype"""
    lib.wann_index_create.restype = ctypes.c_void_p
    x = np.zeros((8, 4), dtype=np.float32)
    labels = np.arange(8, dtype=np.float32)
    lib.wann_index_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_int]
    assert lib.wann_index_create(0, 0, 6, x.ctypes.data, 8, 4, labels.ctypes.data, 4, 2.0, 0.5, None, 0, 1) is None


def test_byte_rows_kernels_register_budget(wa):
    """the one-byte unit's k_search<METRIC, KIND, 6> kernels (3 kernels x 2 metrics) and k_brute_staged for both metrics: no
    scratch segment, and within the register budget of the float32 launch shapes they reuse (at most 256 registers: two
    four-wave workgroups per CU)"""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "dt_w8"], capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0 or not out.stdout.strip():
        pytest.skip("ROCm llvm tools not present")
    lines = out.stdout.splitlines()
    search = [l for l in lines if "k_search" in l]
    assert len(search) == 6 and all("ELi6EEEv" in l for l in search)
    assert len(lines) >= 8  # (+ k_brute_staged for both metrics)
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256, l
        assert int(l.split("scratch")[1].split()[0]) == 0, l
