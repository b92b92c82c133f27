"""Bfloat16 point sets (include/wann.h WANN_DTYPE_BF16 = 5) without a GPU: the Python surface, the rounding rule against two
independent references, the dtype codes the C ABI accepts, the harness switch, the host builder's cache files -- byte-identical
to the float32 build on the points rounded to bfloat16 -- and the register budget of the bfloat16 kernels."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

WANN_DTYPE_F32, WANN_DTYPE_BF16 = 0, 5
KIND_TREE_VAMANA, KIND_SUPER = 3, 4
CLASSES = ("PrefilterIndex", "PostfilterVamanaIndex", "RangeFilterTreeIndex", "VamanaRangeFilterTreeIndex",
           "SuperOptimizedPostfilterTreeIndex")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    lib.wann_abi_version.restype = ctypes.c_int
    return lib


def _build(lib, kind, metric, dtype, X, labels, cache, R, L, cutoff=300, split=2.0, shift=0.5):
    X = np.ascontiguousarray(X)
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    bp = _BuildParams(R, L, 1.0, cache.encode())
    return lib.wann_build_cache_shard(kind, metric, dtype, X.ctypes.data, X.shape[0], X.shape[1], labels.ctypes.data, cutoff,
                                      split, shift, ctypes.byref(bp), 0, 1, 4)


def _read(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _numpy_bits(x):
    """round to nearest, ties to even, on the 16 dropped bits (non-NaN input)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _torch_bits(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_bfloat16_classes_and_helpers_exist(wa):
    for cls in CLASSES:
        for metric in ("Euclidian", "Mips"):
            assert hasattr(wa, f"{cls}BFloat16{metric}"), f"{cls}BFloat16{metric}"
    assert hasattr(wa, "bfloat16_round") and hasattr(wa, "bfloat16_bits")
    for opt in ("set_dense_windows", "dense_window_counters"):
        assert hasattr(wa.PrefilterIndexBFloat16Euclidian, opt)
    assert hasattr(wa.VamanaRangeFilterTreeIndexBFloat16Mips, "set_exact_windows")


def test_bfloat16_bits_random_patterns_match_numpy_and_torch(wa):
    rng = np.random.default_rng(11)
    x = _f32(rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32))
    x = x[~np.isnan(x)]
    got = wa.bfloat16_bits(x)
    assert got.dtype == np.uint16 and got.shape == x.shape
    assert np.array_equal(got, _numpy_bits(x))
    assert np.array_equal(got, _torch_bits(x))


def test_bfloat16_bits_ties_overflow_and_specials(wa):
    cases = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82,       # exact ties: down to the even one, up to the even one
             0xBF808000: 0xBF80, 0xBF818000: 0xBF82,
             0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80,
             0x7F7F7FFF: 0x7F7F, 0x7F7F8000: 0x7F80,       # the last value that stays finite; the first that rounds to inf
             0xFF7F7FFF: 0xFF7F, 0xFF7F8000: 0xFF80, 0x7F7FFFFF: 0x7F80,
             0x00000000: 0x0000, 0x80000000: 0x8000, 0x7F800000: 0x7F80, 0xFF800000: 0xFF80,
             0x00000001: 0x0000, 0x00008000: 0x0000, 0x00008001: 0x0001, 0x00018000: 0x0002,  # float32 subnormals
             0x007FFFFF: 0x0080, 0x80400000: 0x8040, 0x00010000: 0x0001}
    x = _f32(list(cases))
    got = wa.bfloat16_bits(x)
    assert [int(v) for v in got] == list(cases.values())
    assert np.array_equal(got, _numpy_bits(x))
    assert np.array_equal(got, _torch_bits(x))
    # a NaN comes out quiet, its sign kept (signalling and quiet, either sign, payload in the dropped bits only)
    nan_in = _f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA00000, 0xFFFFFFFF])
    nan_out = wa.bfloat16_bits(nan_in)
    for i, o in zip(nan_in.view(np.uint32), nan_out):
        assert (int(o) & 0x7FC0) == 0x7FC0 and (int(o) >> 15) == (int(i) >> 31), (hex(i), hex(o))
    assert np.isnan(wa.bfloat16_round(nan_in)).all()  # (torch's NaN pattern depends on its build: no reference for this one)


def test_bfloat16_round_is_the_widened_bits_and_idempotent(wa):
    rng = np.random.default_rng(12)
    x = _f32(rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)).reshape(1000, 100)
    r = wa.bfloat16_round(x)
    assert r.dtype == np.float32 and r.shape == x.shape
    assert np.array_equal(r.view(np.uint32), wa.bfloat16_bits(x).astype(np.uint32) << 16)
    assert np.array_equal(wa.bfloat16_round(r).view(np.uint32), r.view(np.uint32))
    # VALUES are rounded, whatever the array's dtype: an integer array is never read as bit patterns
    ints = np.array([[0, 1, 257, 16256, 65535]], dtype=np.uint16)
    assert np.array_equal(wa.bfloat16_round(ints), wa.bfloat16_round(ints.astype(np.float32)))
    assert wa.bfloat16_round(ints)[0].tolist() == [0.0, 1.0, 256.0, 16256.0, 65536.0]
    assert np.array_equal(wa.bfloat16_round(np.array([1.0 + 2.0 ** -9], dtype=np.float64)), np.array([1.0], dtype=np.float32))


def _bf16_points(wa, n, d, seed, metric):
    """bfloat16 values over the whole range, as (float32 upcast, uint16 bits): unit-scale values (inner product) or integer-like
    ones (L2), with bfloat16 subnormals, signed zeros, and magnitudes far outside binary16's range planted in a few rows"""
    rng = np.random.default_rng(seed)
    if metric == 1:
        X = rng.standard_normal((n, d)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    else:
        X = np.rint(rng.standard_normal((n, d)) * 40 + 100).astype(np.float32)
    rows = rng.choice(n, 40, replace=False)
    X[rows[:10], :4] = _f32([0x00010000, 0x007F0000, 0x80030000, 0x00400000])  # bfloat16 subnormals
    X[rows[10:20], 1] = -0.0
    X[rows[20:30], 2] = 0.0
    X[rows[30:], 3:7] = np.array([2.0 ** 40, -(2.0 ** 40), 3.0e-30, 70000.0], dtype=np.float32)
    R = wa.bfloat16_round(X)
    return R, wa.bfloat16_bits(X)


@pytest.mark.parametrize("kind,metric,R,n,d", [(KIND_TREE_VAMANA, 0, 24, 1500, 20), (KIND_TREE_VAMANA, 1, 24, 1500, 33),
                                               (KIND_SUPER, 0, 24, 1500, 16), (KIND_SUPER, 1, 24, 1500, 40),
                                               (KIND_TREE_VAMANA, 1, 96, 900, 24)],  # R = 96: the host builder's wide rows
                         ids=["tree-l2", "tree-mips", "super-l2", "super-mips", "tree-mips-R96"])
def test_bfloat16_cache_files_equal_float32_on_rounded_rows(wa, lib, tmp_path, kind, metric, R, n, d):
    X32, bits = _bf16_points(wa, n, d, 7 + kind + metric, metric)
    assert np.array_equal(X32.view(np.uint32), bits.astype(np.uint32) << 16)
    labels = ((np.random.default_rng(5).permutation(n) + 0.5) / n).astype(np.float32)
    bdir, fdir = str(tmp_path / "bf16") + "/", str(tmp_path / "single") + "/"
    os.makedirs(bdir), os.makedirs(fdir)
    assert _build(lib, kind, metric, WANN_DTYPE_BF16, bits, labels, bdir, R, 2 * R) == 0, lib.wann_last_error()
    assert _build(lib, kind, metric, WANN_DTYPE_F32, X32, labels, fdir, R, 2 * R) == 0, lib.wann_last_error()
    bf, ff = _read(bdir), _read(fdir)
    assert bf and list(bf) == list(ff)
    for f in bf:
        assert bf[f] == ff[f], f"graph file {f} differs"


@pytest.mark.parametrize("dtype", [4, 6])
def test_unassigned_dtype_codes_are_refused(lib, tmp_path, dtype):
    """5 is bfloat16; 4 stays unassigned and 6 is past the end -- both are refused by name"""
    X = np.zeros((100, 8), dtype=np.float32)
    labels = np.linspace(0, 1, 100, dtype=np.float32)
    assert _build(lib, KIND_TREE_VAMANA, 0, dtype, X, labels, str(tmp_path) + "/", 16, 32) != 0
    assert b"dtype" in lib.wann_last_error()
    assert os.listdir(tmp_path) == []
    assert lib.wann_abi_version() == 5  # an addition only


def test_raw_beam_search_typed_dtype_codes(wa):
    """the pybind entry refuses 4 and 6 before it touches a device, and takes dtype 5 points as uint16 bit patterns only"""
    g = np.zeros((4, 3), dtype=np.int32)
    q = np.zeros((1, 8), dtype=np.float32)
    for dtype in (4, 6, -1):
        with pytest.raises(RuntimeError, match="unknown dtype"):
            wa.raw_beam_search_typed(0, dtype, np.zeros((4, 8), dtype=np.float32), g, 0, q, np.zeros(1, dtype=np.int64), 4)
    with pytest.raises(RuntimeError, match="uint16"):
        wa.raw_beam_search_typed(0, 5, np.zeros((4, 8), dtype=np.float32), g, 0, q, np.zeros(1, dtype=np.int64), 4)


def test_harness_constructors_resolve_bfloat16_only_with_the_opt_in(wa):
    from rangefilteredann_amd import harness
    assert harness.vamana_range_filter_tree_constructor("mips", "bfloat16", float16=True) is wa.VamanaRangeFilterTreeIndexBFloat16Mips
    assert (harness.super_optimized_postfilter_tree_constructor("Euclidian", "bfloat16", float16=True)
            is wa.SuperOptimizedPostfilterTreeIndexBFloat16Euclidian)
    assert harness.postfilter_vamana_constructor("Euclidian", "bfloat16", float16=True) is wa.PostfilterVamanaIndexBFloat16Euclidian
    assert harness.prefilter_index_constructor("mips", "bfloat16", float16=True) is wa.PrefilterIndexBFloat16Mips
    for cons in (harness.prefilter_index_constructor, harness.postfilter_vamana_constructor,
                 harness.vamana_range_filter_tree_constructor, harness.super_optimized_postfilter_tree_constructor):
        with pytest.raises(Exception, match="Invalid data type"):
            cons("mips", "bfloat16")
    x = np.array([[1.0 + 2.0 ** -9, 3.0e38]], dtype=np.float32)
    assert np.array_equal(harness.round_to_dtype(x, "bfloat16"), wa.bfloat16_round(x))
    assert harness.round_to_dtype(x, "float") is x


def test_harness_cache_directory_and_results_prefix(wa, tmp_path):
    from rangefilteredann_amd import harness
    s = harness.Settings(dataset_folder=str(tmp_path), cache_root=str(tmp_path / "c"), results_dir=str(tmp_path / "r"), dtype="bfloat16")
    e = harness.Experiments(s)
    assert e._cache("ds/") == os.path.join(str(tmp_path / "c"), "bfloat16", "ds/") and os.path.isdir(e._cache("ds/"))
    path = e.save_results([("2pow-3", "prefiltering", 1.0, 2.0)], "ds")
    assert os.path.basename(path) == "bfloat16_ds_results.csv"


def _resources(pattern):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), pattern], capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0 or not out.stdout.strip():
        pytest.skip("ROCm llvm tools not present")
    return out.stdout.splitlines()


def test_bfloat16_kernels_register_budget(wa):
    """the bfloat16 units' kernels: k_search<METRIC, KIND, 5> (3 kernels x 2 metrics) and k_brute for both metrics, the eight
    k_gemm_scores<STRIDE> instantiations -- no scratch segment, at most 256 registers (two four-wave workgroups per CU)"""
    lines = _resources("dt_bf16")
    search = [l for l in lines if "k_search" in l]
    assert len(search) == 6 and all("ELi5EEEv" in l for l in search)
    assert len([l for l in lines if "k_brute" in l]) == 2
    gemm = [l for l in lines if "k_gemm_scores" in l]
    assert len(gemm) == 8, gemm
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256, l
        assert int(l.split("scratch")[1].split()[0]) == 0, l
