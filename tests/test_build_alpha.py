"""CPU: the graph builders where test_host_build.py does not reach -- alpha != 1, uint8 / int8 rows and hub nodes.
(1) The oracle's builder and the product's host builder each reproduce, name and bytes, the files the REAL reference wrote
(tests/golden/build_alpha_golden.npz).  (2) Host builder == oracle builder on trees at alpha = 1.2 and on byte trees.
(3) The hub inputs of the GPU tests (util.star_hub) really are hubs: in the oracle-built graph at least 0.9 n rows of a
partition hold the hub placed at its start point -- a condition on the input, far below the measured 0.9995."""
import ctypes
import os

import numpy as np
import pytest

import golden_util as gu
from util import distinct_labels, random_rows, sift_like, star_hub, tree_hub_ids, unit_mixture

DTYPE = {"Float": 0, "UInt8": 1, "Int8": 2}  # WANN_DTYPE_* (include/wann.h)
KIND = {"PostfilterVamanaIndex": 1, "VamanaRangeFilterTreeIndex": 3, "SuperOptimizedPostfilterTreeIndex": 4}


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


def _elem(sfx):
    return "UInt8" if sfx.startswith("UInt8") else "Int8" if sfx.startswith("Int8") else "Float"


def _host_build(wa, lib, kind, sfx, X, labels, cache, R, L, alpha, cutoff=1000, split=2.0, shift=0.5):
    """the product's host builder: floats through the Python build_cache_shard, byte rows through the C ABI with their dtype"""
    metric = 1 if sfx.endswith("Mips") else 0
    if _elem(sfx) == "Float":
        wa.build_cache_shard(KIND[kind], metric, X, labels, cutoff, split, shift, wa.BuildParams(R, L, alpha, cache), 0, 1, 4)
        return
    X = np.ascontiguousarray(X)
    assert X.dtype == (np.uint8 if _elem(sfx) == "UInt8" else np.int8)
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    bp = _BuildParams(R, L, alpha, cache.encode())
    rc = lib.wann_build_cache_shard(KIND[kind], metric, DTYPE[_elem(sfx)], X.ctypes.data, X.shape[0], X.shape[1], labels.ctypes.data,
                                    cutoff, split, shift, ctypes.byref(bp), 0, 1, 4)
    assert rc == 0, lib.wann_last_error()


def _oracle_build(oracle, kind, sfx, X, labels, cache, R, L, alpha, **kw):
    labkw = "filters" if kind == "PostfilterVamanaIndex" else "filter_values"
    return getattr(oracle, kind + sfx)(X, **{labkw: labels}, build_params=oracle.BuildParams(R, L, alpha, cache), threads=4, **kw)


def _read(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _ref_ties(monkeypatch, mode="1"):
    monkeypatch.setenv("WANN_REF_TIES", mode)
    monkeypatch.setenv("ORC_REF_TIES", mode)


@pytest.mark.parametrize("name", gu.BUILD_ALPHA_CASES)
def test_builders_write_the_references_graph_file(oracle, wa, lib, tmp_path, monkeypatch, name):
    """alpha = 1.2 and 1.175, the four byte types (reference tie order) and the hub input: the oracle's builder and the host
    builder each write the file the REAL reference wrote, name and bytes."""
    c = gu.build_alpha_case(name)
    _ref_ties(monkeypatch)
    pdir, odir = str(tmp_path / "product") + "/", str(tmp_path / "oracle") + "/"
    os.makedirs(pdir), os.makedirs(odir)
    _oracle_build(oracle, "PostfilterVamanaIndex", c["sfx"], c["X"], c["labels"], odir, c["R"], c["L"], c["alpha"])
    _host_build(wa, lib, "PostfilterVamanaIndex", c["sfx"], c["X"], c["labels"], pdir, c["R"], c["L"], c["alpha"])
    for who, d in (("oracle", odir), ("host", pdir)):
        assert os.listdir(d) == [c["file_name"]], who
        assert open(d + c["file_name"], "rb").read() == c["file"], f"{who} builder: graph differs from the reference's"


def test_alpha_changes_the_fixture_graphs():
    """(the alpha fixtures are not the alpha = 1 graph under another name: a builder that ignores alpha fails them)"""
    base = gu.load_build()["gauss_l2|file"].tobytes()
    a, b = gu.build_alpha_case("gauss_l2_a120")["file"], gu.build_alpha_case("gauss_l2_a1175")["file"]
    assert len({base, a, b}) == 3
    assert gu.build_alpha_case("i8_mips")["file"] != gu.build_alpha_case("i8_mips_a120")["file"]


TREES = [
    ("VamanaRangeFilterTreeIndex", "FloatEuclidian", 1.2, dict(cutoff=300, split_factor=2)),
    ("SuperOptimizedPostfilterTreeIndex", "FloatMips", 1.2, dict(cutoff=300, split_factor=2, shift_factor=0.5)),
    ("VamanaRangeFilterTreeIndex", "Int8Mips", 1.0, dict(cutoff=300, split_factor=2)),
    ("VamanaRangeFilterTreeIndex", "UInt8Euclidian", 1.0, dict(cutoff=300, split_factor=2)),
]


@pytest.mark.parametrize("kind,sfx,alpha,kw", TREES)
def test_host_builder_matches_oracle_builder_on_trees(oracle, wa, lib, tmp_path, monkeypatch, kind, sfx, alpha, kw):
    n, d, R, L = 3000, 24, 16, 32
    if _elem(sfx) == "Float":
        X = (unit_mixture if sfx.endswith("Mips") else sift_like)(n, d, 19)(n)
    else:
        X = random_rows(sfx, np.random.default_rng(19), n, d)
    labels = distinct_labels(n, 7)
    _ref_ties(monkeypatch)
    pdir, odir = str(tmp_path / "product") + "/", str(tmp_path / "oracle") + "/"
    os.makedirs(pdir), os.makedirs(odir)
    oidx = _oracle_build(oracle, kind, sfx, X, labels, odir, R, L, alpha, **kw)
    _host_build(wa, lib, kind, sfx, X, labels, pdir, R, L, alpha, kw["cutoff"], kw["split_factor"], kw.get("shift_factor", 0.5))
    pf, of = _read(pdir), _read(odir)
    assert list(pf) == list(of) and len(pf) == sum(oidx.levels()) > 1
    for f in pf:
        assert pf[f] == of[f], f"graph file {f} differs"


# ------------------------------------------------------------------------------------------
# the hub inputs are hubs
# ------------------------------------------------------------------------------------------
def _rows_holding(rows, node):
    deg = rows[:, 0:1]
    return int(((rows[:, 1:] == node) & (np.arange(rows.shape[1] - 1)[None, :] < deg)).any(1).sum())


@pytest.mark.parametrize("metric,d", [("mips", 32), ("l2", 64)])
@pytest.mark.parametrize("alpha", [1.0, 1.2])
def test_star_hub_is_in_nearly_every_row(oracle, monkeypatch, metric, d, alpha):
    n = 12000
    _ref_ties(monkeypatch)
    hub = int(oracle.random_permutation(n)[0])
    X = star_hub(n, d, metric, [hub])
    rows = oracle.vamana_build(oracle.pad_rows(X), d, 1 if metric == "mips" else 0, 0, n, 16, 16, alpha)
    assert _rows_holding(rows, hub) >= 0.9 * n


def test_star_hub_byte_rows(oracle, tmp_path, monkeypatch):
    n = 12000
    _ref_ties(monkeypatch)
    hub = int(oracle.random_permutation(n)[0])
    X = star_hub(n, 32, "mips", [hub], elem=np.uint8)
    assert X.dtype == np.uint8 and X.max() == 255 and np.delete(X, hub, 0).max() == 15
    idx = _oracle_build(oracle, "PostfilterVamanaIndex", "UInt8Mips", X, np.arange(n, dtype=np.float32), str(tmp_path) + "/", 16, 16, 1.0)
    assert _rows_holding(idx.partition_graph(0, 0), hub) >= 0.9 * n


def test_star_hub_tree_has_a_hub_in_the_root_and_in_both_halves(oracle, tmp_path, monkeypatch):
    """one hub per partition of 24 000 and 12 000 points (norms 8, 4, 4 over disjoint dimensions); the 6 000-point leaves have
    none of their own"""
    n = 24000
    _ref_ties(monkeypatch)
    hubs = tree_hub_ids(oracle, n)
    X = star_hub(n, 32, "mips", hubs, norms=(8.0, 4.0, 4.0))
    idx = _oracle_build(oracle, "VamanaRangeFilterTreeIndex", "FloatMips", X, np.arange(n, dtype=np.float32), str(tmp_path) + "/",
                        16, 16, 1.0, cutoff=6000, split_factor=2)
    assert idx.levels() == [1, 2, 4]
    for (lv, i), hub in zip(((0, 0), (1, 0), (1, 1)), hubs):
        a, b = idx.partition_range(lv, i)
        assert a <= hub < b
        assert _rows_holding(idx.partition_graph(lv, i), hub - a) >= 0.9 * (b - a), (lv, i)
