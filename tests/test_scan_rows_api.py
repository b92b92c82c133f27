"""CPU: the surface of the switch that lets the exact scans of a float32 index read its shadow rows (include/wann.h,
wann_set_scan_rows): the three C symbols, their behaviour on a null index, the unchanged ABI version, the header, and the
Python methods on the float32 classes of the five index families."""
import ctypes
import os
import re

import pytest

from util import REPO

SYMBOLS = ("wann_set_scan_rows", "wann_scan_rows", "wann_last_scan_rows")
FAMILIES = ("PrefilterIndex", "PostfilterVamanaIndex", "RangeFilterTreeIndex", "VamanaRangeFilterTreeIndex", "SuperOptimizedPostfilterTreeIndex")


@pytest.fixture(scope="module")
def lib(wa):
    import rangefilteredann_amd
    return ctypes.CDLL(rangefilteredann_amd.lib_path())


def test_symbols_are_exported_and_the_abi_version_stays(wa, lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.wann_abi_version() == 5 and wa.abi_version() == 5


def test_a_null_index(lib):
    """a negative error for the setter, whose non-negative values are settings; no setting and no store to report"""
    lib.wann_set_scan_rows.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.wann_set_scan_rows.restype = ctypes.c_int
    for f in (lib.wann_scan_rows, lib.wann_last_scan_rows):
        f.argtypes = [ctypes.c_void_p]
        f.restype = ctypes.c_int
    assert lib.wann_set_scan_rows(None, 1) < 0
    assert lib.wann_set_scan_rows(None, 0) < 0
    assert lib.wann_scan_rows(None) == 0 and lib.wann_last_scan_rows(None) == 0


def test_header_declares_the_three_calls_and_keeps_the_counters():
    with open(os.path.join(REPO, "include", "wann.h")) as f:
        h = f.read()
    assert re.search(r"int wann_set_scan_rows\(wann_index \*\w+, int on\);", h)
    assert re.search(r"int wann_scan_rows\(const wann_index \*\w+\);", h)
    assert re.search(r"int wann_last_scan_rows\(const wann_index \*\w+\);", h)
    assert "#define WANN_ABI_VERSION 5" in h
    # wann_counters is what ABI 5 says it is: the scan's store is reported by a call of its own
    c = re.search(r"typedef struct \{([^}]*)\} wann_counters;", h).group(1)
    fields = re.findall(r"(?:int64_t|double) (\w+);", c)
    assert fields[0] == "beam_searches" and fields[-1] == "lookaheads_issued" and len(fields) == 24
    assert "scan_rows" not in fields


def test_python_methods_on_the_float32_classes_of_the_five_families(wa):
    for family in FAMILIES:
        for sfx in ("FloatEuclidian", "FloatMips"):
            cls = getattr(wa, family + sfx)
            assert callable(getattr(cls, "set_scan_rows")) and callable(getattr(cls, "scan_rows")), (family, sfx)
            assert callable(getattr(cls, "set_byte_rows")), (family, sfx)  # (the classes that have the one have the other)
