"""CPU: the surface of the wide call and of the refined call's stop_k (include/wann.h WIDE ROWS / REFINED SEARCH): the four C
symbols and their prototypes, the unchanged ABI version, their answers to a null index, the Python methods on the five index
families with their keywords, and the register / scratch figures of every k_search the stop_k field went into."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from util import REPO

SYMBOLS = ("wann_batch_search_device_wide", "wann_batch_search_wide", "wann_batch_search_device_refined_stop", "wann_batch_search_refined_stop")
FAMILIES = ("PrefilterIndex", "PostfilterVamanaIndex", "RangeFilterTreeIndex", "VamanaRangeFilterTreeIndex", "SuperOptimizedPostfilterTreeIndex")


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
    assert ("int wann_batch_search_device_wide(wann_index *index, const void *d_queries, const float *d_ranges, int64_t nq, "
            "int64_t query_id_base, const char *method, const wann_query_params *qp, int64_t width, uint32_t *d_ids, float *d_dists, "
            "void *hip_stream);") in flat
    assert ("int wann_batch_search_wide(wann_index *index, const void *queries, const float *ranges, int64_t nq, const char *method, "
            "const wann_query_params *qp, int64_t width, uint32_t *ids, float *dists);") in flat
    assert ("int wann_batch_search_device_refined_stop(wann_index *index, const void *d_queries, const float *d_ranges, int64_t nq, "
            "int64_t query_id_base, const char *method, const wann_query_params *qp, int64_t refine_k, int64_t stop_k, uint32_t *d_ids, "
            "float *d_dists, void *hip_stream);") in flat
    assert ("int wann_batch_search_refined_stop(wann_index *index, const float *queries, const float *ranges, int64_t nq, "
            "const char *method, const wann_query_params *qp, int64_t refine_k, int64_t stop_k, uint32_t *ids, float *dists);") in flat
    assert "#define WANN_ABI_VERSION 5" in h
    # the public parameter struct did not change: no stop_k or width in it
    qp = re.search(r"typedef struct \{([^}]*)\} wann_query_params;", h).group(1)
    fields = re.findall(r"(?:int64_t|int32_t|int|double|float) (\w+);", qp)
    assert fields[0] == "k" and "beam_width" in fields and "stop_k" not in fields and "width" not in fields, fields


def test_a_null_index(lib):
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.wann_batch_search_device_wide.argtypes = [vp, vp, vp, i64, i64, ctypes.c_char_p, vp, i64, vp, vp, vp]
    lib.wann_batch_search_wide.argtypes = [vp, vp, vp, i64, ctypes.c_char_p, vp, i64, vp, vp]
    lib.wann_batch_search_device_refined_stop.argtypes = [vp, vp, vp, i64, i64, ctypes.c_char_p, vp, i64, i64, vp, vp, vp]
    lib.wann_batch_search_refined_stop.argtypes = [vp, vp, vp, i64, ctypes.c_char_p, vp, i64, i64, vp, vp]
    for name in SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    assert lib.wann_batch_search_device_wide(None, None, None, 0, 0, b"", None, 40, None, None, None) == -1
    assert lib.wann_batch_search_wide(None, None, None, 0, b"", None, 40, None, None) == -1
    assert lib.wann_batch_search_device_refined_stop(None, None, None, 0, 0, b"", None, 40, 20, None, None, None) == -1
    assert lib.wann_batch_search_refined_stop(None, None, None, 0, b"", None, 40, 20, None, None) == -1


def test_python_methods_on_the_five_families(wa):
    for family in FAMILIES:
        for sfx in ("FloatEuclidian", "UInt8Mips", "Float16Mips", "BFloat16Euclidian", "Float8Mips"):
            cls = getattr(wa, family + sfx)
            for name in ("batch_search_wide", "batch_search_device_wide"):
                assert callable(getattr(cls, name)), (family, sfx, name)
            doc = cls.batch_search_wide.__doc__  # two forms: with and without a method, as batch_search has across the families
            assert doc.count("width:") == 2 and doc.count("query_method: str") == 1, doc
            assert re.search(r"query_params: \S+, width: [^,]+, ids_ptr:", cls.batch_search_device_wide.__doc__)
            for name in ("batch_search_refined", "batch_search_device_refined"):  # a trailing keyword, None = the call as it was
                assert re.search(r"\*, stop_k: [^,)]*None = None\)", getattr(cls, name).__doc__), getattr(cls, name).__doc__


def test_search_kernels_keep_their_registers(wa):
    """every k_search of the eight units (48 kernels): no scratch segment and no spilled vector register with the stop_k field in
    its arguments, and the float32 unit's k_search<0, 0> still fits its 256 registers (profiles/refine_stop_kernel_resources.txt)"""
    llvm = "/opt/rocm/lib/llvm/bin"  # (what the tool runs: without them there is nothing to read the code objects with)
    if not all(os.path.exists(os.path.join(llvm, t)) for t in ("clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm llvm tools not present")
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_search"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and out.stdout.strip(), out.stderr[-800:]  # (a broken tool or a missing library is a failure, not a skip)
    lines = out.stdout.splitlines()
    assert len(lines) == 48, len(lines)
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256, l
        assert int(l.split("scratch")[1].split()[0]) == 0, l
        assert int(l.split(" spill")[1].split()[0]) == 0, l
