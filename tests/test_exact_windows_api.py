"""CPU: the surface of the exact-windows option of the graph-backed tree indexes: the two C symbols, the unchanged ABI version,
the header's struct, the pybind methods on the two class families (and on no other), and a harness that sets the limit only
where the option exists and only when it is non-zero."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("queries", "dense_queries", "unproven", "rescued", "passes", "rows_scanned")
SUFFIXES = ("FloatEuclidian", "FloatMips", "Float16Euclidian", "Float16Mips", "UInt8Euclidian", "UInt8Mips", "Int8Euclidian", "Int8Mips")


def test_library_exports_the_symbols_and_keeps_its_abi_version(wa):
    import rangefilteredann_amd
    lib = ctypes.CDLL(os.path.join(os.path.dirname(rangefilteredann_amd.__file__), "libwann.so"))
    assert lib.wann_abi_version() == 5 and wa.abi_version() == 5
    lib.wann_set_exact_windows.restype = ctypes.c_int64
    lib.wann_set_exact_windows.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.wann_get_exact_window_counters.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    # (no device needed: a null index is refused -- with a NEGATIVE code by the setter, whose non-negative values are limits)
    assert lib.wann_set_exact_windows(None, 4096) == -1
    assert lib.wann_set_exact_windows(None, 0) < 0
    assert lib.wann_get_exact_window_counters(None, None) == 1


def test_header_declares_the_struct_and_both_calls():
    with open(os.path.join(REPO, "include", "wann.h")) as f:
        h = f.read()
    m = re.search(r"typedef struct \{([^}]*)\} wann_exact_window_counters;", h)
    assert m, "wann_exact_window_counters is not declared"
    assert tuple(re.findall(r"int64_t (\w+);", m.group(1))) == FIELDS
    assert re.search(r"int64_t wann_set_exact_windows\(wann_index \*\w+, int64_t max_points\);", h)
    assert re.search(r"int wann_get_exact_window_counters\(const wann_index \*\w+, wann_exact_window_counters \*\w+\);", h)
    assert "#define WANN_ABI_VERSION 5" in h
    # wann_counters is what ABI 5 says it is: the new counters live in a struct of their own
    c = re.search(r"typedef struct \{([^}]*)\} wann_counters;", h).group(1)
    fields = re.findall(r"(?:int64_t|double) (\w+);", c)
    assert fields[0] == "beam_searches" and fields[-1] == "lookaheads_issued" and len(fields) == 24
    assert not any(f in fields for f in FIELDS if f != "queries") and "exact_queries" not in fields


def test_pybind_methods_on_the_two_graph_backed_tree_families_only(wa):
    for sfx in SUFFIXES:
        for family in ("VamanaRangeFilterTreeIndex", "SuperOptimizedPostfilterTreeIndex"):
            cls = getattr(wa, family + sfx)
            assert callable(getattr(cls, "set_exact_windows")) and callable(getattr(cls, "exact_window_counters")), (family, sfx)
        for family in ("PrefilterIndex", "PostfilterVamanaIndex", "RangeFilterTreeIndex"):
            cls = getattr(wa, family + sfx)
            assert not hasattr(cls, "set_exact_windows") and not hasattr(cls, "exact_window_counters"), (family, sfx)


def test_harness_sets_the_limit_only_where_it_exists_and_only_when_non_zero(tmp_path):
    from rangefilteredann_amd import harness as hz

    class With:
        def __init__(self):
            self.calls = []

        def set_exact_windows(self, max_points):
            self.calls.append(max_points)
            return 0

    class Without:
        __slots__ = ()  # (any attribute the harness tried to set would raise)

    w = With()
    assert hz.use_exact_windows(w, 4096) is w and w.calls == [4096]
    w0 = With()
    assert hz.use_exact_windows(w0, 0) is w0 and hz.use_exact_windows(w0) is w0 and w0.calls == []
    plain = Without()
    assert hz.use_exact_windows(plain, 4096) is plain
    assert hz.Settings(dataset_folder="x").exact_windows == 0
    # the limit is part of the results file's name: runs with and without it do not overwrite each other
    rows = [("2pow-3", "optimized-postfiltering_1.000_2_10_1", 1.0, 2.0, 1.0, 2, 0)]
    off = hz.Experiments(hz.Settings(dataset_folder="x", results_dir=str(tmp_path))).save_results(rows, "sift")
    on = hz.Experiments(hz.Settings(dataset_folder="x", results_dir=str(tmp_path), exact_windows=4096)).save_results(rows, "sift")
    assert off != on and "4096" in os.path.basename(on) and "4096" not in os.path.basename(off)
    assert os.path.basename(off) == "sift_results.csv"
