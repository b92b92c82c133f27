"""Float16 point sets (include/wann.h WANN_DTYPE_F16) without a GPU: the Python surface, the harness switch, and the host
builder's cache files, which must be byte-identical to the float32 build on the points upcast to float32 -- the property
that lets the float16 and float32 indexes share a graph cache and return the same rows."""
import ctypes
import os

import numpy as np
import pytest

WANN_DTYPE_F32, WANN_DTYPE_F16 = 0, 3
KIND_TREE_VAMANA, KIND_SUPER = 3, 4
CLASSES = ("PrefilterIndex", "PostfilterVamanaIndex", "RangeFilterTreeIndex", "VamanaRangeFilterTreeIndex",
           "SuperOptimizedPostfilterTreeIndex")


class _BuildParams(ctypes.Structure):
    _fields_ = [("max_degree", ctypes.c_int64), ("limit", ctypes.c_int64), ("alpha", ctypes.c_double),
                ("cache_path", ctypes.c_char_p)]


@pytest.fixture(scope="module")
def lib(wa):
    import rangefilteredann_amd
    lib = ctypes.CDLL(rangefilteredann_amd.lib_path())
    lib.wann_build_cache_shard.restype = ctypes.c_int
    lib.wann_build_cache_shard.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_double,
                                           ctypes.POINTER(_BuildParams), ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.wann_last_error.restype = ctypes.c_char_p
    return lib


def _build(lib, kind, metric, dtype, X, labels, cache, R, L, cutoff=300, split=2.0, shift=0.5):
    X = np.ascontiguousarray(X)
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    bp = _BuildParams(R, L, 1.0, cache.encode())
    rc = lib.wann_build_cache_shard(kind, metric, dtype, X.ctypes.data, X.shape[0], X.shape[1], labels.ctypes.data, cutoff,
                                    split, shift, ctypes.byref(bp), 0, 1, 4)
    return rc


def _read(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _half_points(n, d, seed, metric):
    """float16 rows over the whole range: unit-scale values (inner product) or integer-like ones (L2), with fp16 subnormals,
    signed zeros and values near the largest finite half (65504) planted in a few rows"""
    rng = np.random.default_rng(seed)
    if metric == 1:
        X = rng.standard_normal((n, d)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    else:
        X = np.rint(rng.standard_normal((n, d)) * 40 + 100).astype(np.float32)
    X16 = X.astype(np.float16)
    sub = np.array([2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15, -(2.0 ** -20), 1023 * 2.0 ** -24], dtype=np.float16)
    assert (np.abs(sub.astype(np.float32)) < 2.0 ** -14).all()  # all fp16 subnormals
    rows = rng.choice(n, 40, replace=False)
    X16[rows[:10], : len(sub)] = sub
    X16[rows[10:20], 1] = np.float16(-0.0)
    X16[rows[20:30], 2] = np.float16(0.0)
    big = np.array([65504, -65504, 65472, 60000], dtype=np.float16)
    X16[rows[30:], 3: 3 + len(big)] = big
    return X16


def test_float16_classes_exist(wa):
    for cls in CLASSES:
        for metric in ("Euclidian", "Mips"):
            assert hasattr(wa, f"{cls}Float16{metric}"), f"{cls}Float16{metric}"
    assert hasattr(wa, "raw_beam_search_typed")


def test_harness_constructors_resolve_float16(wa):
    """float16 is asked for explicitly (float16=True, what --dtype float16 passes); by default the constructors keep the
    reference wrapper's "Invalid data type" for it"""
    from rangefilteredann_amd import harness
    assert harness.vamana_range_filter_tree_constructor("mips", "float16", float16=True) is wa.VamanaRangeFilterTreeIndexFloat16Mips
    assert (harness.super_optimized_postfilter_tree_constructor("Euclidian", "float16", float16=True)
            is wa.SuperOptimizedPostfilterTreeIndexFloat16Euclidian)
    assert harness.postfilter_vamana_constructor("Euclidian", "float16", float16=True) is wa.PostfilterVamanaIndexFloat16Euclidian
    assert harness.prefilter_index_constructor("mips", "float16", float16=True) is wa.PrefilterIndexFloat16Mips
    assert harness.prefilter_index_constructor("mips", "float", float16=True) is wa.PrefilterIndexFloatMips
    with pytest.raises(Exception, match="Invalid data type"):
        harness.vamana_range_filter_tree_constructor("mips", "float16")


@pytest.mark.parametrize("kind,metric,R,n,d", [(KIND_TREE_VAMANA, 0, 24, 1500, 20), (KIND_TREE_VAMANA, 1, 24, 1500, 33),
                                               (KIND_SUPER, 0, 24, 1500, 16), (KIND_SUPER, 1, 24, 1500, 40),
                                               (KIND_TREE_VAMANA, 1, 96, 900, 24)],  # R = 96: the host builder's wide rows
                         ids=["tree-l2", "tree-mips", "super-l2", "super-mips", "tree-mips-R96"])
def test_float16_cache_files_equal_float32_on_upcast_rows(lib, tmp_path, kind, metric, R, n, d):
    X16 = _half_points(n, d, 7 + kind + metric, metric)
    labels = ((np.random.default_rng(5).permutation(n) + 0.5) / n).astype(np.float32)
    hdir, fdir = str(tmp_path / "half") + "/", str(tmp_path / "single") + "/"
    os.makedirs(hdir), os.makedirs(fdir)
    assert _build(lib, kind, metric, WANN_DTYPE_F16, X16, labels, hdir, R, 2 * R) == 0, lib.wann_last_error()
    assert _build(lib, kind, metric, WANN_DTYPE_F32, X16.astype(np.float32), labels, fdir, R, 2 * R) == 0, lib.wann_last_error()
    hf, ff = _read(hdir), _read(fdir)
    assert hf and list(hf) == list(ff)
    for f in hf:
        assert hf[f] == ff[f], f"graph file {f} differs"


def test_unknown_dtype_is_refused(lib, tmp_path):
    X = np.zeros((100, 8), dtype=np.float32)
    labels = np.linspace(0, 1, 100, dtype=np.float32)
    assert _build(lib, KIND_TREE_VAMANA, 0, 4, X, labels, str(tmp_path) + "/", 16, 32) != 0
    assert b"dtype" in lib.wann_last_error()
    assert os.listdir(tmp_path) == []


def test_float16_search_kernels_register_budget(wa):
    """the float16 unit's k_search<METRIC, KIND, 3> kernels: no scratch segment, and within the register budget of the
    float32 launch shapes they reuse (at most 256 registers: two four-wave workgroups per CU)"""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                                       "kernel_resources.py"), "dt_f16"], capture_output=True, text=True, timeout=300)
    if out.returncode != 0 or not out.stdout.strip():
        pytest.skip("ROCm llvm tools not present")
    lines = out.stdout.splitlines()
    search = [l for l in lines if "k_search" in l]
    assert len(search) == 6 and all("ELi3EEEv" in l for l in search)  # (3 kernels x 2 metrics)
    assert len(lines) >= 8  # (+ k_brute for both metrics)
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256, l
        assert int(l.split("scratch")[1].split()[0]) == 0, l
