"""CPU: the layout of the device copy of the one-byte shadow rows as a pure function of the C ABI (include/wann.h
wann_byte_row_position; window_ann.byte_row_position).  Inside every aligned group of 32 elements the bytes are permuted so that
the four 4-element blocks 8 b + 4 h, b = 4 c .. 4 c + 3, of lane h of a lane pair are the 16 contiguous bytes at 32 c + 16 h."""
import ctypes
import os

import pytest

from util import REPO


@pytest.fixture(scope="module")
def lib(wa):
    import rangefilteredann_amd
    L = ctypes.CDLL(rangefilteredann_amd.lib_path())
    L.wann_byte_row_position.restype = ctypes.c_int64
    L.wann_byte_row_position.argtypes = [ctypes.c_int64]
    return L


def _formula(e):
    return 32 * (e >> 5) + 16 * ((e >> 2) & 1) + 4 * ((e >> 3) & 3) + (e & 3)


def test_symbol_header_and_abi_version(lib):
    assert hasattr(lib, "wann_byte_row_position")
    assert lib.wann_abi_version() == 5
    header = open(os.path.join(REPO, "include", "wann.h")).read()
    assert "int64_t wann_byte_row_position(int64_t element);" in header


def test_the_formula(lib):
    for e in range(4096):
        assert lib.wann_byte_row_position(e) == _formula(e), e
    assert lib.wann_byte_row_position(-1) == -1
    assert lib.wann_byte_row_position(-(2 ** 40)) == -1
    assert lib.wann_byte_row_position(2 ** 40 + 4) == 2 ** 40 + 16  # (64-bit throughout)


def test_every_group_of_32_maps_onto_itself(lib):
    for g in range(4096 // 32):
        got = sorted(lib.wann_byte_row_position(e) for e in range(32 * g, 32 * g + 32))
        assert got == list(range(32 * g, 32 * g + 32)), g


def test_a_lane_s_four_blocks_are_sixteen_contiguous_bytes(lib):
    """b = 4 c + i < 512, h < 2: block 8 b + 4 h starts at 32 c + 16 h + 4 i and its four elements follow one another"""
    for c in range(128):
        for h in range(2):
            for i in range(4):
                first = 8 * (4 * c + i) + 4 * h
                assert [lib.wann_byte_row_position(first + j) for j in range(4)] == [32 * c + 16 * h + 4 * i + j for j in range(4)], (c, h, i)


def test_the_python_wrapper_agrees(wa, lib):
    assert wa.byte_row_position(-1) == -1 and wa.byte_row_position(-7) == -1
    for e in range(4096):
        assert wa.byte_row_position(e) == lib.wann_byte_row_position(e) == _formula(e), e
