"""GPU: graphs of degree 65 .. 128 are built by the GPU builder's two-half kernels (wann_build_kernels_body.inc, HALVES = 2), not
by the host builder.  Every case builds once on the GPU and once with WANN_HOST_BUILD=1: same file names and bytes, the GPU
builder's summary line on stderr, rows of more than 64 neighbours in the files (a condition on the inputs: weakly prunable
points -- alpha = 1.2 under L2 --, checked on the CPU with the oracle's builder when they were chosen), and no degree above R."""
import os
import re

import numpy as np
import pytest

from util import distinct_labels, random_rows, star_hub

pytestmark = pytest.mark.gpu
TREE = "VamanaRangeFilterTreeIndex"
POST = "PostfilterVamanaIndex"
SUMMARY = re.compile(r"\[wann gpu build\] \d+ partitions.*second reverse pass: (\d+) groups in (\d+) rounds")
TREE_KW = dict(cutoff=200, split_factor=2)
N = 1500


def _gauss(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _case(oracle, name):
    """(kind, suffix, points, labels, R, L, alpha, index keywords, host suffix, environment)"""
    lab = distinct_labels(N, 91)
    if name.startswith("degree"):  # one slot in the second half; rs = 80, 96; rs = 128 with a dead slot; full rows
        R = int(name[6:])
        return TREE, "FloatEuclidian", _gauss(N, 32, 90), lab, R, 2 * R, 1.2, TREE_KW, None, {}
    if name.startswith("ties"):  # bytes 0 .. 3: most distances repeat, the tie order decides the files
        X = np.random.default_rng(92).integers(0, 4, (N, 24)).astype(np.uint8)
        return TREE, "UInt8Euclidian", X, lab, 96, 192, 1.2, TREE_KW, None, {"WANN_REF_TIES": name[4:]}
    if name == "mips_alpha":  # (inner product: distances are negative, alpha < 1 is the weak prune)
        X = random_rows("FloatMips", np.random.default_rng(93), N, 64)
        return TREE, "FloatMips", X, lab, 96, 192, 0.9, TREE_KW, None, {}
    if name == "hub":  # batches of 160 sources + a row of 96 > the LDS buffer of 2 * 32 + 64 + 96 keys; L = 32: the seen table in LDS
        n = 8000
        X = star_hub(n, 32, "mips", [int(oracle.random_permutation(n)[0])])
        return POST, "FloatMips", X, np.arange(n, dtype=np.float32), 96, 32, 1.0, {}, None, {}
    if name == "restart":  # 256 - 96 slots: visited lists of beam 192 do not fit, the second attempt's 512 - 96 do
        return TREE, "FloatEuclidian", _gauss(N, 32, 94), lab, 96, 192, 1.2, TREE_KW, None, {"WANN_BUILD_VIS_CAP": "256"}
    if name == "float16":
        X = _gauss(N, 33, 95).astype(np.float16).astype(np.float32)
        return TREE, "Float16Euclidian", X, lab, 96, 192, 1.2, TREE_KW, "FloatEuclidian", {}
    raise KeyError(name)


CASES = ["degree65", "degree80", "degree96", "degree127", "degree128", "ties1", "ties0", "mips_alpha", "hub", "restart", "float16"]


def _read(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _build_both(oracle, wa, monkeypatch, tmp_path, capfd, name):
    """the GPU-built and the host-built index, the GPU build's files and its stderr; asserts what every case asserts"""
    kind, sfx, X, labels, R, L, alpha, kw, host_sfx, env = _case(oracle, name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("WANN_VERBOSE", "1")
    labkw = "filters" if kind == POST else "filter_values"
    gdir, hdir = str(tmp_path / "gpu") + "/", str(tmp_path / "host") + "/"
    os.makedirs(gdir), os.makedirs(hdir)
    monkeypatch.delenv("WANN_HOST_BUILD", raising=False)
    capfd.readouterr()
    gidx = getattr(wa, kind + sfx)(X, **{labkw: labels}, build_params=wa.BuildParams(R, L, alpha, gdir), **kw)
    err = capfd.readouterr().err
    monkeypatch.setenv("WANN_HOST_BUILD", "1")
    hidx = getattr(wa, kind + (host_sfx or sfx))(X, **{labkw: labels}, build_params=wa.BuildParams(R, L, alpha, hdir), **kw)
    monkeypatch.delenv("WANN_HOST_BUILD")
    gf, hf = _read(gdir), _read(hdir)
    assert list(gf) == list(hf) and len(gf) > 0
    for f in gf:
        assert gf[f] == hf[f], f"{f}: GPU-built graph differs from the host-built one"
    assert SUMMARY.search(err), "no summary line of the GPU builder on stderr: the graphs were not built on the GPU"
    widest = 0
    for f, blob in gf.items():
        hdr = np.frombuffer(blob[:8], dtype=np.int32)
        deg = np.frombuffer(blob[8:8 + 4 * hdr[0]], dtype=np.int32)
        assert hdr[1] == R and 0 <= deg.min() and deg.max() <= R, f
        widest = max(widest, int(deg.max()))
    assert widest > 64, "input too prunable: no row reaches the second half"
    return gidx, hidx, err


@pytest.mark.parametrize("name", CASES)
def test_wide_gpu_builder_matches_host_builder(oracle, wa, gpu, tmp_path, monkeypatch, capfd, name):
    _, _, err = _build_both(oracle, wa, monkeypatch, tmp_path, capfd, name)
    groups = sum(int(g) for g, _ in SUMMARY.findall(err))
    if name == "hub":  # the global-scratch prune of a wide row ran
        assert groups > 0
    if name == "restart":
        assert err.count("restarting the GPU build") >= 1


def test_wide_rows_built_into_the_pool_search_like_uploaded_ones(oracle, wa, gpu, tmp_path, monkeypatch, capfd):
    """the builder writes straight into the adjacency pool, host builds are uploaded through convert_rows: same answers, bit for bit"""
    gidx, hidx, _ = _build_both(oracle, wa, monkeypatch, tmp_path, capfd, "degree96")
    nq = 64
    Q = _gauss(nq, 32, 96)
    W = np.tile(np.array([[-1.0, 2.0]]), (nq, 1))
    qp = wa.QueryParams(10, 100, 1.35, 10**7, 10**4, 2, 10000, None, False)
    gi, gd = gidx.batch_search(Q, W, nq, "optimized_postfilter", qp)
    hi, hd = hidx.batch_search(Q, W, nq, "optimized_postfilter", qp)
    assert np.array_equal(gi, hi) and np.array_equal(gd.view(np.uint32), hd.view(np.uint32))
