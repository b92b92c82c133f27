"""CPU: the surface of the refined search (include/wann.h REFINED SEARCH): the five C symbols and their prototypes, the unchanged
ABI version and wann_counters, their answers to a null index, the Python methods on the five index families, the numpy
restatement the GPU tests compare against, and the register / scratch figures of the new kernel unit."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import refine_util
from util import REPO

SYMBOLS = ("wann_set_refine_rows", "wann_refine_rows_bytes", "wann_batch_search_device_refined", "wann_batch_search_refined",
           "wann_get_refine_counters")
FAMILIES = ("PrefilterIndex", "PostfilterVamanaIndex", "RangeFilterTreeIndex", "VamanaRangeFilterTreeIndex", "SuperOptimizedPostfilterTreeIndex")
METHODS = ("set_refine_rows", "refine_rows_bytes", "batch_search_refined", "batch_search_device_refined", "refine_counters")


@pytest.fixture(scope="module")
def lib(wa):
    import rangefilteredann_amd
    return ctypes.CDLL(rangefilteredann_amd.lib_path())


def test_symbols_header_and_abi_version(wa, lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.wann_abi_version() == 5 and wa.abi_version() == 5
    with open(os.path.join(REPO, "include", "wann.h")) as f:
        h = f.read()
    flat = re.sub(r"\s+", " ", h)
    assert "int wann_set_refine_rows(wann_index *index, const float *points, int64_t n, int64_t d);" in flat
    assert "int64_t wann_refine_rows_bytes(const wann_index *index);" in flat
    assert ("int wann_batch_search_device_refined(wann_index *index, const void *d_queries, const float *d_ranges, int64_t nq, "
            "int64_t query_id_base, const char *method, const wann_query_params *qp, int64_t refine_k, uint32_t *d_ids, "
            "float *d_dists, void *hip_stream);") in flat
    assert ("int wann_batch_search_refined(wann_index *index, const float *queries, const float *ranges, int64_t nq, "
            "const char *method, const wann_query_params *qp, int64_t refine_k, uint32_t *ids, float *dists);") in flat
    assert "int wann_get_refine_counters(const wann_index *index, wann_refine_counters *out);" in flat
    assert "#define WANN_ABI_VERSION 5" in h
    c = re.search(r"typedef struct \{([^}]*)\} wann_counters;", h).group(1)
    fields = re.findall(r"(?:int64_t|double) (\w+);", c)
    assert fields[0] == "beam_searches" and fields[-1] == "lookaheads_issued" and len(fields) == 24
    assert not [f for f in fields if "refine" in f]
    r = re.search(r"typedef struct \{([^}]*)\} wann_refine_counters;", h).group(1)
    assert re.findall(r"(?:int64_t|double) (\w+);", r) == ["refined_queries", "refined_rows", "refine_ms"]


def test_a_null_index(lib):
    """negative errors from the setter, both searches and the counters' getter; -1 bytes"""
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.wann_set_refine_rows.argtypes = [vp, vp, i64, i64]
    lib.wann_refine_rows_bytes.argtypes = [vp]
    lib.wann_refine_rows_bytes.restype = i64
    lib.wann_batch_search_device_refined.argtypes = [vp, vp, vp, i64, i64, ctypes.c_char_p, vp, i64, vp, vp, vp]
    lib.wann_batch_search_refined.argtypes = [vp, vp, vp, i64, ctypes.c_char_p, vp, i64, vp, vp]
    lib.wann_get_refine_counters.argtypes = [vp, vp]
    for f in (lib.wann_set_refine_rows, lib.wann_batch_search_device_refined, lib.wann_batch_search_refined, lib.wann_get_refine_counters):
        f.restype = ctypes.c_int
    rows = (ctypes.c_float * 4)(1, 2, 3, 4)
    out = (ctypes.c_int64 * 3)()
    assert lib.wann_set_refine_rows(None, rows, 2, 2) < 0
    assert lib.wann_set_refine_rows(None, None, 0, 0) < 0
    assert lib.wann_refine_rows_bytes(None) == -1
    assert lib.wann_batch_search_device_refined(None, None, None, 0, 0, b"", None, 10, None, None, None) < 0
    assert lib.wann_batch_search_refined(None, None, None, 0, b"", None, 10, None, None) < 0
    assert lib.wann_get_refine_counters(None, out) < 0


def test_python_methods_on_the_five_families(wa):
    for family in FAMILIES:
        for sfx in ("FloatEuclidian", "Float16Mips", "BFloat16Euclidian", "Float8Mips"):
            cls = getattr(wa, family + sfx)
            for name in METHODS:
                assert callable(getattr(cls, name)), (family, sfx, name)


def test_refine_reference_self_test(oracle):
    refine_util.self_test(oracle)


def test_refine_kernels_have_no_scratch(wa):
    """k_refine<0> (squared L2) and k_refine<1> (inner product): no scratch segment, no spilled vector register"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_refine"], capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0 or not out.stdout.strip():
        pytest.skip("ROCm llvm tools not present")
    lines = out.stdout.splitlines()
    assert sorted(re.search(r"k_refineILi(\d)E", l).group(1) for l in lines) == ["0", "1"], lines
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256, l
        assert int(l.split("scratch")[1].split()[0]) == 0, l
        assert int(l.split(" spill")[1].split()[0]) == 0, l
