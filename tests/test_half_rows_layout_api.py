"""CPU: the layout of the device copy of the half shadow rows as a pure function of the C ABI (include/wann.h
wann_half_row_position; window_ann.half_row_position).  Inside every aligned group of 16 elements the halves are permuted so
that the two 4-element blocks 8 b + 4 h, b = 2 c and 2 c + 1, of lane h of a lane pair are the 16 contiguous bytes at byte
32 c + 16 h of the row -- and the kernel unit that reads the copy (wann_kernels_h16.hip) within its register budget."""
import ctypes
import os

import pytest

from util import REPO


@pytest.fixture(scope="module")
def lib(wa):
    import rangefilteredann_amd
    L = ctypes.CDLL(rangefilteredann_amd.lib_path())
    L.wann_half_row_position.restype = ctypes.c_int64
    L.wann_half_row_position.argtypes = [ctypes.c_int64]
    return L


def _formula(e):
    return 16 * (e >> 4) + 8 * ((e >> 2) & 1) + 4 * ((e >> 3) & 1) + (e & 3)


def test_symbol_header_and_abi_version(lib):
    assert hasattr(lib, "wann_half_row_position")
    assert lib.wann_abi_version() == 5
    header = open(os.path.join(REPO, "include", "wann.h")).read()
    assert "int64_t wann_half_row_position(int64_t element);" in header


def test_the_positions_the_layout_names(lib):
    for e, p in ((0, 0), (4, 8), (8, 4), (12, 12), (16, 16)):
        assert lib.wann_half_row_position(e) == p, e
    assert lib.wann_half_row_position(-1) == -1
    assert lib.wann_half_row_position(-(2 ** 40)) == -1
    assert lib.wann_half_row_position(2 ** 40 + 4) == 2 ** 40 + 8  # (64-bit throughout)


def test_the_rule_repeats_every_16_elements(lib):
    for e in range(4096):
        assert lib.wann_half_row_position(e) == 16 * (e // 16) + lib.wann_half_row_position(e % 16) == _formula(e), e


def test_every_group_of_16_maps_onto_itself(lib):
    for g in range(4096 // 16):
        got = sorted(lib.wann_half_row_position(e) for e in range(16 * g, 16 * g + 16))
        assert got == list(range(16 * g, 16 * g + 16)), g


def test_a_lane_s_two_blocks_are_sixteen_contiguous_bytes(lib):
    """position(16 c + 8 i + 4 h + j) = 16 c + 8 h + 4 i + j: block b = 2 c + i of lane h starts at half 16 c + 8 h + 4 i"""
    for c in range(256):
        for h in range(2):
            for i in range(2):
                for j in range(4):
                    assert lib.wann_half_row_position(16 * c + 8 * i + 4 * h + j) == 16 * c + 8 * h + 4 * i + j, (c, h, i, j)


def test_the_python_wrapper_agrees(wa, lib):
    assert wa.half_row_position(-1) == -1 and wa.half_row_position(-7) == -1
    for e in range(4096):
        assert wa.half_row_position(e) == lib.wann_half_row_position(e) == _formula(e), e


def test_the_view_type_is_not_a_public_dtype(lib):
    """7 is the internal view type of the paired rows: wann_index_create refuses it as it refuses 6"""
    import numpy as np
    lib.wann_index_create.restype = ctypes.c_void_p
    lib.wann_index_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    x = np.zeros((8, 4), dtype=np.float32)
    labels = np.arange(8, dtype=np.float32)
    assert lib.wann_index_create(0, 0, 7, x.ctypes.data, 8, 4, labels.ctypes.data, 4, 2.0, 0.5, None, 0, 1) is None


def test_half_rows_kernels_register_budget(wa):
    """the paired unit's k_search<METRIC, KIND, 7> kernels (3 kernels x 2 metrics) and k_brute for both metrics: no scratch
    segment, and within the register budget of the float16 launch shapes they reuse (at most 256 registers: two four-wave
    workgroups per CU)"""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "dt_h16"], capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0:
        pytest.skip("ROCm llvm tools not present")
    lines = out.stdout.splitlines()
    search = [l for l in lines if "k_search" in l]
    brute = [l for l in lines if "k_brute" in l]
    assert len(search) == 6 and all("ELi7EEEv" in l for l in search)
    assert len(brute) == 2 and len(lines) == 8
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256, l
        assert int(l.split("scratch")[1].split()[0]) == 0, l
        assert int(l.split(" spill")[1].split()[0]) == 0, l
