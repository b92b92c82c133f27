"""Float8 point sets (include/wann.h WANN_DTYPE_F8 = 8, OCP E4M3) without a GPU: the Python surface, the rounding rule and the
decode table against torch's CPU conversion (the independent reference), the dtype codes the C ABI accepts, the refusal of NaN
patterns, the harness switch, the host builder's cache files -- byte-identical to the float32 build on the points rounded to
float8 -- and the register budget of the float8 kernels."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

WANN_DTYPE_F32, WANN_DTYPE_F8 = 0, 8
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


def _torch_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def _torch_table():
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()


def _same_bits(got, ref, x):
    """equal patterns; where the reference gives a NaN pattern: a NaN pattern, and the sign of the input kept"""
    nan = (ref & 0x7F) == 0x7F
    assert np.array_equal(got[~nan], ref[~nan])
    assert ((got[nan] & 0x7F) == 0x7F).all()
    assert np.array_equal(got[nan] >> 7, (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)[nan] >> 31).astype(np.uint8))


def test_float8_classes_and_helpers_exist(wa):
    for cls in CLASSES:
        for metric in ("Euclidian", "Mips"):
            assert hasattr(wa, f"{cls}Float8{metric}"), f"{cls}Float8{metric}"
    assert hasattr(wa, "float8_round") and hasattr(wa, "float8_bits")
    for opt in ("set_dense_windows", "dense_window_counters"):
        assert hasattr(wa.PrefilterIndexFloat8Euclidian, opt)
    assert hasattr(wa.VamanaRangeFilterTreeIndexFloat8Mips, "set_exact_windows")
    assert hasattr(wa.SuperOptimizedPostfilterTreeIndexFloat8Euclidian, "exact_window_counters")


def test_float8_bits_random_patterns_match_torch(wa):
    rng = np.random.default_rng(11)
    x = _f32(rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32))
    got = wa.float8_bits(x)
    assert got.dtype == np.uint8 and got.shape == x.shape
    _same_bits(got, _torch_bits(x), x)
    # ... and on magnitudes inside the format's range, where nearly every pattern is finite
    y = (x.view(np.uint32) & np.uint32(0x80FFFFFF) | (rng.integers(115, 137, x.shape).astype(np.uint32) << 23)).view(np.float32)
    ref = _torch_bits(y)
    assert ((ref & 0x7F) != 0x7F).mean() > 0.9
    _same_bits(wa.float8_bits(y), ref, y)


def test_float8_bits_edge_table_matches_torch(wa):
    tab = _torch_table()
    fin = [b for b in range(0x7F)]
    edges = [448.0, 464.0, 465.0, 479.9, 480.0, 1e30, 2.0 ** -9, -(2.0 ** -9), 2.0 ** -10, 2.0 ** -10 * 1.01, 2.0 ** -10 * 0.99,
             3 * 2.0 ** -10, 0.0, -0.0, np.inf, -np.inf, 2.0 ** -6, 2.0 ** -6 - 2.0 ** -10, 2.0 ** -6 - 2.0 ** -11]
    for b in fin[:-1]:  # the tie between every pair of neighbours (binade boundaries included) and its float32 neighbours
        mid = np.float32(0.5) * (tab[b] + tab[b + 1])
        edges += [mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1e9))]
    x = np.array(edges, dtype=np.float32)
    x = np.concatenate([x, -x, _f32([1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000])])  # both signs; float32 subnormals
    got = wa.float8_bits(x)
    _same_bits(got, _torch_bits(x), x)
    assert [int(v) for v in wa.float8_bits(np.array([448, 464, 465, 2.0 ** -10, 2.0 ** -10 * 1.01, -465, -0.0], dtype=np.float32))] == \
        [0x7E, 0x7E, 0x7F, 0x00, 0x01, 0xFF, 0x80]
    nan_out = wa.float8_bits(_f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001]))
    assert [int(v) for v in nan_out] == [0x7F, 0xFF, 0x7F, 0xFF]


def test_float8_decode_equals_torch_table(wa):
    tab = _torch_table()
    pats = np.arange(256, dtype=np.uint8)
    fin = (pats & 0x7F) != 0x7F
    assert np.array_equal(wa.float8_bits(tab[fin]), pats[fin])                       # every finite value is its own rounding
    assert np.array_equal(wa.float8_round(tab[fin]).view(np.uint32), tab[fin].view(np.uint32))  # and decodes to torch's bits
    assert np.isnan(wa.float8_round(tab[~fin])).all() and np.isnan(tab[~fin]).all()
    assert tab[fin].max() == 448.0 and np.abs(tab[fin][tab[fin] != 0]).min() == 2.0 ** -9


def test_float8_round_is_the_widened_bits_and_idempotent(wa):
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((1000, 100)) * np.exp2(rng.uniform(-12, 8, (1000, 1)))).astype(np.float32)
    x = np.clip(x, -448, 448)
    r = wa.float8_round(x)
    assert r.dtype == np.float32 and r.shape == x.shape
    assert np.array_equal(r.view(np.uint32), _torch_table()[wa.float8_bits(x)].view(np.uint32))
    assert np.array_equal(wa.float8_round(r).view(np.uint32), r.view(np.uint32))
    # VALUES are rounded, whatever the array's dtype: a uint8 array is never read as bit patterns
    ints = np.array([[0, 1, 17, 126, 255]], dtype=np.uint8)
    assert np.array_equal(wa.float8_round(ints), wa.float8_round(ints.astype(np.float32)))
    assert wa.float8_round(ints)[0].tolist() == [0.0, 1.0, 16.0, 128.0, 256.0]
    assert np.array_equal(wa.float8_round(np.array([1.0 + 2.0 ** -5], dtype=np.float64)), np.array([1.0], dtype=np.float32))


def _f8_points(wa, n, d, seed, metric):
    """float8 values over the whole range, as (float32 upcast, uint8 bits): unit-scale values (inner product) or integer-like ones
    (L2), with subnormals, signed zeros and +-448 planted in a few rows"""
    rng = np.random.default_rng(seed)
    if metric == 1:
        X = rng.standard_normal((n, d)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    else:
        X = np.rint(rng.standard_normal((n, d)) * 40 + 100).astype(np.float32)
    rows = rng.choice(n, 40, replace=False)
    X[rows[:10], :4] = np.array([2.0 ** -9, -3 * 2.0 ** -9, 7 * 2.0 ** -9, 2.0 ** -10 * 1.5], dtype=np.float32)  # subnormals
    X[rows[10:20], 1] = -0.0
    X[rows[20:30], 2] = 0.0
    X[rows[30:], 3:7] = np.array([448.0, -448.0, 464.0, 2.0 ** -6], dtype=np.float32)
    bits = wa.float8_bits(X)
    assert ((bits & 0x7F) != 0x7F).all()
    return wa.float8_round(X), bits


@pytest.mark.parametrize("kind,metric,R,n,d", [(KIND_TREE_VAMANA, 0, 24, 1500, 20), (KIND_TREE_VAMANA, 1, 24, 1500, 33),
                                               (KIND_SUPER, 0, 24, 1500, 16), (KIND_SUPER, 1, 24, 1500, 40),
                                               (KIND_TREE_VAMANA, 1, 96, 900, 20)],  # R = 96: the host builder's wide rows
                         ids=["tree-l2", "tree-mips", "super-l2", "super-mips", "tree-mips-R96"])
def test_float8_cache_files_equal_float32_on_rounded_rows(wa, lib, tmp_path, kind, metric, R, n, d):
    X32, bits = _f8_points(wa, n, d, 7 + kind + metric, metric)
    assert np.array_equal(X32.view(np.uint32), _torch_table()[bits].view(np.uint32))
    assert (np.abs(X32) == 448).any() and np.signbit(X32[X32 == 0]).any() and (np.abs(X32)[X32 != 0] < 2.0 ** -6).any()
    labels = ((np.random.default_rng(5).permutation(n) + 0.5) / n).astype(np.float32)
    bdir, fdir = str(tmp_path / "f8") + "/", str(tmp_path / "single") + "/"
    os.makedirs(bdir), os.makedirs(fdir)
    assert _build(lib, kind, metric, WANN_DTYPE_F8, bits, labels, bdir, R, 2 * R) == 0, lib.wann_last_error()
    assert _build(lib, kind, metric, WANN_DTYPE_F32, X32, labels, fdir, R, 2 * R) == 0, lib.wann_last_error()
    bf, ff = _read(bdir), _read(fdir)
    assert bf and list(bf) == list(ff)
    for f in bf:
        assert bf[f] == ff[f], f"graph file {f} differs"


@pytest.mark.parametrize("pattern", [0x7F, 0xFF])
def test_float8_nan_patterns_are_refused_before_the_cache_is_touched(wa, lib, tmp_path, pattern):
    _, bits = _f8_points(wa, 400, 16, 3, 1)
    bits = bits.copy()
    bits[137, 5] = pattern
    bits[300, 0] = pattern
    labels = np.linspace(0, 1, 400, dtype=np.float32)
    assert _build(lib, KIND_TREE_VAMANA, 1, WANN_DTYPE_F8, bits, labels, str(tmp_path) + "/", 16, 32) == 1  # WANN_ERR_INVALID
    msg = lib.wann_last_error().decode()
    assert "row 137" in msg and "NaN" in msg, msg
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("dtype", [4, 6, 7, 9])
def test_other_dtype_codes_stay_refused(lib, tmp_path, dtype):
    """8 is float8; 4 stays unassigned, 6 and 7 stay internal view types, 9 is past the end -- all refused by name"""
    X = np.zeros((100, 8), dtype=np.float32)
    labels = np.linspace(0, 1, 100, dtype=np.float32)
    assert _build(lib, KIND_TREE_VAMANA, 0, dtype, X, labels, str(tmp_path) + "/", 16, 32) != 0
    assert b"dtype" in lib.wann_last_error()
    assert os.listdir(tmp_path) == []
    assert lib.wann_abi_version() == 5  # an addition only


def test_raw_beam_search_typed_takes_float8_as_uint8_only(wa):
    g = np.zeros((4, 3), dtype=np.int32)
    q = np.zeros((1, 8), dtype=np.float32)
    for dtype in (4, 6, 7, 9):
        with pytest.raises(RuntimeError, match="unknown dtype"):
            wa.raw_beam_search_typed(0, dtype, np.zeros((4, 8), dtype=np.float32), g, 0, q, np.zeros(1, dtype=np.int64), 4)
    for pts in (np.zeros((4, 8), dtype=np.float32), np.zeros((4, 8), dtype=np.int8), np.zeros((4, 8), dtype=np.uint16)):
        with pytest.raises(RuntimeError, match="uint8"):
            wa.raw_beam_search_typed(0, 8, pts, g, 0, q, np.zeros(1, dtype=np.int64), 4)


def test_harness_constructors_resolve_float8_only_with_the_opt_in(wa):
    from rangefilteredann_amd import harness
    assert harness.vamana_range_filter_tree_constructor("mips", "float8", float16=True) is wa.VamanaRangeFilterTreeIndexFloat8Mips
    assert (harness.super_optimized_postfilter_tree_constructor("Euclidian", "float8", float16=True)
            is wa.SuperOptimizedPostfilterTreeIndexFloat8Euclidian)
    assert harness.postfilter_vamana_constructor("Euclidian", "float8", float16=True) is wa.PostfilterVamanaIndexFloat8Euclidian
    assert harness.prefilter_index_constructor("mips", "float8", float16=True) is wa.PrefilterIndexFloat8Mips
    for cons in (harness.prefilter_index_constructor, harness.postfilter_vamana_constructor,
                 harness.vamana_range_filter_tree_constructor, harness.super_optimized_postfilter_tree_constructor):
        with pytest.raises(Exception, match="Invalid data type"):
            cons("mips", "float8")
    x = np.array([[1.0 + 2.0 ** -5, 300.0, 2.0 ** -10]], dtype=np.float32)
    assert np.array_equal(harness.round_to_dtype(x, "float8"), wa.float8_round(x))
    assert harness.round_to_dtype(x, "float8")[0].tolist() == [1.0, 288.0, 0.0]
    assert harness.round_to_dtype(x, "float") is x


def test_harness_cache_directory_and_results_prefix(wa, tmp_path):
    from rangefilteredann_amd import harness
    s = harness.Settings(dataset_folder=str(tmp_path), cache_root=str(tmp_path / "c"), results_dir=str(tmp_path / "r"), dtype="float8")
    e = harness.Experiments(s)
    assert e._cache("ds/") == os.path.join(str(tmp_path / "c"), "float8", "ds/") and os.path.isdir(e._cache("ds/"))
    path = e.save_results([("2pow-3", "prefiltering", 1.0, 2.0)], "ds")
    assert os.path.basename(path) == "float8_ds_results.csv"


def _resources(pattern):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), pattern], capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0 or not out.stdout.strip():
        pytest.skip("ROCm llvm tools not present")
    return out.stdout.splitlines()


def test_float8_kernels_register_budget(wa):
    """the float8 units' kernels: k_search<METRIC, KIND, 8> (3 kernels x 2 metrics), k_brute and k_brute_staged for both metrics,
    k_point_norms, k_rerank and k_rerank_cover for both metrics, the eight k_gemm_scores<STRIDE> instantiations -- no scratch
    segment, at most 256 registers"""
    lines = _resources("dt_f8")
    search = [l for l in lines if "k_search" in l]
    assert len(search) == 6 and all("ELi8EEEv" in l for l in search)
    assert len([l for l in lines if "k_brute_staged" in l]) == 2
    assert len([l for l in lines if "7k_bruteI" in l]) == 2
    assert len([l for l in lines if "k_gemm_scores" in l]) == 8
    assert len([l for l in lines if "k_point_norms" in l]) == 1
    assert len([l for l in lines if "k_rerank" in l]) == 4
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256, l
        assert int(l.split("scratch")[1].split()[0]) == 0, l
