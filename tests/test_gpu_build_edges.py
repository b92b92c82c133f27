"""GPU: the Vamana build kernels (wann_gpu_build.cpp, wann_build_kernels_body.inc and its uint8 / int8 units) where
test_gpu_parity.py does not reach: alpha != 1 in the prune, every byte unit, hub nodes whose reverse-edge group goes to the
second reverse pass, compact point types against the HOST builder, the restart after a visited-list overflow inside a tree of
partitions, and the degrees around the wave width.  Every case builds once on the GPU and once with WANN_HOST_BUILD=1 and asks
for the same file names and bytes (the host builder equals the oracle's and the real reference's: test_build_alpha.py); where
the REAL reference's file is stored (tests/golden/build_alpha_golden.npz) the GPU's file must equal that too."""
import os
import re

import numpy as np
import pytest

import golden_util as gu
from util import distinct_labels, random_rows, sift_like, star_hub, tree_hub_ids, unit_mixture

pytestmark = pytest.mark.gpu
TREE = "VamanaRangeFilterTreeIndex"
POST = "PostfilterVamanaIndex"
SECOND_PASS = re.compile(r"second reverse pass: (\d+) groups in (\d+) rounds")


def _read(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _gpu_and_host(wa, monkeypatch, tmp_path, kind, sfx, X, labels, R, L, alpha, kw=None, host_sfx=None):
    """build on the GPU and with the host builder (of host_sfx, when the GPU index is a compact type); the files are equal,
    names and bytes.  Returns the GPU build's files."""
    labkw = "filters" if kind == POST else "filter_values"
    gdir, hdir = str(tmp_path / "gpu") + "/", str(tmp_path / "host") + "/"
    os.makedirs(gdir), os.makedirs(hdir)
    monkeypatch.delenv("WANN_HOST_BUILD", raising=False)
    getattr(wa, kind + sfx)(X, **{labkw: labels}, build_params=wa.BuildParams(R, L, alpha, gdir), **(kw or {}))
    monkeypatch.setenv("WANN_HOST_BUILD", "1")
    getattr(wa, kind + (host_sfx or sfx))(X, **{labkw: labels}, build_params=wa.BuildParams(R, L, alpha, hdir), **(kw or {}))
    monkeypatch.delenv("WANN_HOST_BUILD")
    gf, hf = _read(gdir), _read(hdir)
    assert list(gf) == list(hf) and len(gf) > 0
    for f in gf:
        assert gf[f] == hf[f], f"{f}: GPU-built graph differs from the host-built one"
    return gf


def _second_pass(err):
    """(groups, rounds) the GPU builder sent to its second reverse pass, summed over the WANN_VERBOSE summary lines"""
    found = SECOND_PASS.findall(err)
    assert found, "no summary line of the GPU builder on stderr"
    print("second reverse pass (groups, rounds):", found)
    return sum(int(g) for g, _ in found), sum(int(r) for _, r in found)


# ------------------------------------------------------------------------------------------
# the reference's files: alpha != 1, the four byte types, the hub input
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gu.BUILD_ALPHA_CASES)
def test_gpu_builder_writes_the_references_file(wa, gpu, tmp_path, monkeypatch, capfd, name):
    c = gu.build_alpha_case(name)
    monkeypatch.setenv("WANN_REF_TIES", "1")
    monkeypatch.setenv("WANN_VERBOSE", "1")
    gf = _gpu_and_host(wa, monkeypatch, tmp_path, POST, c["sfx"], c["X"], c["labels"], c["R"], c["L"], c["alpha"])
    assert list(gf) == [c["file_name"]]
    assert gf[c["file_name"]] == c["file"], "GPU-built graph differs from the file the reference wrote"
    groups, rounds = _second_pass(capfd.readouterr().err)
    if name == "star_mips":
        assert groups > 0 and rounds >= 20
    else:  # (batches of at most 18 points: nothing can outgrow the LDS buffer)
        assert (groups, rounds) == (0, 0)


# ------------------------------------------------------------------------------------------
# alpha != 1 on trees, byte rows and the global seen-table path
# ------------------------------------------------------------------------------------------
ALPHA_CASES = [
    (TREE, "FloatEuclidian", sift_like, 128, 6000, dict(cutoff=500, split_factor=2), 32, 64, 1.2),
    (TREE, "FloatEuclidian", sift_like, 128, 6000, dict(cutoff=500, split_factor=2), 32, 64, 0.9),
    (TREE, "FloatMips", unit_mixture, 100, 4000, dict(cutoff=400, split_factor=2), 24, 48, 1.2),
    (TREE, "UInt8Euclidian", sift_like, 64, 3000, dict(cutoff=400, split_factor=2), 24, 48, 1.2),
    (POST, "FloatEuclidian", sift_like, 64, 20000, dict(), 64, 500, 1.2),  # bits > kMaxLdsBits: the seen table in global memory
]


@pytest.mark.parametrize("kind,sfx,gen,d,n,kw,R,L,alpha", ALPHA_CASES)
def test_alpha_gpu_builder_matches_host_builder(wa, gpu, tmp_path, monkeypatch, capfd, kind, sfx, gen, d, n, kw, R, L, alpha):
    X = gen(n, d, 79)(n)
    labels = distinct_labels(n, 15)
    monkeypatch.setenv("WANN_VERBOSE", "1")
    _gpu_and_host(wa, monkeypatch, tmp_path, kind, sfx, X, labels, R, L, alpha, kw)
    # the control of the hub tests: small batches leave the second pass idle
    if n <= 6000:  # (batch + R <= 152: no group can outgrow the LDS buffer of at least 192 candidates)
        assert _second_pass(capfd.readouterr().err) == (0, 0)


# ------------------------------------------------------------------------------------------
# the byte units on trees, in both tie orders
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", ["1", "0"])
@pytest.mark.parametrize("sfx,d", [("Int8Euclidian", 70), ("Int8Mips", 520), ("UInt8Mips", 200)])
def test_byte_trees_gpu_builder_matches_host_builder(wa, gpu, tmp_path, monkeypatch, sfx, d, ties):
    n = 3000
    X = random_rows(sfx, np.random.default_rng(80 + d), n, d)
    labels = distinct_labels(n, 16)
    monkeypatch.setenv("WANN_REF_TIES", ties)
    _gpu_and_host(wa, monkeypatch, tmp_path, TREE, sfx, X, labels, 24, 48, 1.0, dict(cutoff=300, split_factor=2))


# ------------------------------------------------------------------------------------------
# hub nodes: the second reverse pass (A.big, candidates in global scratch)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", ["1", "0"])
@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("sfx,d", [("FloatMips", 32), ("FloatEuclidian", 64)])
def test_hub_goes_through_the_second_reverse_pass(oracle, wa, gpu, tmp_path, monkeypatch, capfd, sfx, d, alpha, ties):
    """one node in (nearly) every row: every batch of 240 inserts is one reverse group of 240 > 192 - 16 candidates, which the
    first pass hands to the second; 50 full batches, so at least 20 rounds must report one"""
    n = 12000
    X = star_hub(n, d, "mips" if sfx.endswith("Mips") else "l2", [int(oracle.random_permutation(n)[0])])
    monkeypatch.setenv("WANN_REF_TIES", ties)
    monkeypatch.setenv("WANN_VERBOSE", "1")
    _gpu_and_host(wa, monkeypatch, tmp_path, POST, sfx, X, np.arange(n, dtype=np.float32), 16, 16, alpha)
    groups, rounds = _second_pass(capfd.readouterr().err)
    assert groups > 0 and rounds >= 20


def test_hubs_of_a_tree_share_second_pass_rounds(oracle, wa, gpu, tmp_path, monkeypatch, capfd):
    """a hub at the start point of the 24 000-point root and of both 12 000-point halves (batches of 480 and 240), none in the
    6 000-point leaves (batches of 120: first pass only): the lock-step rounds carry several second-pass groups at once"""
    n = 24000
    X = star_hub(n, 32, "mips", tree_hub_ids(oracle, n), norms=(8.0, 4.0, 4.0))
    monkeypatch.setenv("WANN_VERBOSE", "1")
    gf = _gpu_and_host(wa, monkeypatch, tmp_path, TREE, "FloatMips", X, np.arange(n, dtype=np.float32), 16, 16, 1.0,
                       dict(cutoff=6000, split_factor=2))
    assert len(gf) == 7
    groups, rounds = _second_pass(capfd.readouterr().err)
    assert rounds > 0 and groups > rounds


def test_byte_hub_goes_through_the_second_reverse_pass(oracle, wa, gpu, tmp_path, monkeypatch, capfd):
    n = 12000
    X = star_hub(n, 32, "mips", [int(oracle.random_permutation(n)[0])], elem=np.uint8)
    monkeypatch.setenv("WANN_REF_TIES", "1")
    monkeypatch.setenv("WANN_VERBOSE", "1")
    _gpu_and_host(wa, monkeypatch, tmp_path, POST, "UInt8Mips", X, np.arange(n, dtype=np.float32), 16, 16, 1.0)
    groups, rounds = _second_pass(capfd.readouterr().err)
    assert groups > 0 and rounds >= 20


# ------------------------------------------------------------------------------------------
# compact point types: the GPU build of the compact index == the HOST build of the float32 index on the rounded points
# ------------------------------------------------------------------------------------------
def _rounded(wa, elem, X):
    if elem == "Float8":
        return wa.float8_round(X)
    if elem == "BFloat16":
        return wa.bfloat16_round(X)
    return X.astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("metric", ["Euclidian", "Mips"])
@pytest.mark.parametrize("elem", ["Float8", "Float16", "BFloat16"])
def test_compact_gpu_build_equals_float32_host_build(wa, gpu, tmp_path, monkeypatch, elem, metric, alpha):
    n, d = 3000, 33
    if metric == "Mips":
        X = unit_mixture(n, d, 81)(n)
    else:
        X = (np.random.default_rng(81).standard_normal((n, d)) * 2).astype(np.float32)
    X = np.ascontiguousarray(_rounded(wa, elem, X), dtype=np.float32)
    assert np.array_equal(_rounded(wa, elem, X), X)
    _gpu_and_host(wa, monkeypatch, tmp_path, TREE, elem + metric, X, distinct_labels(n, 17), 16, 32, alpha,
                  dict(cutoff=300, split_factor=2), host_sfx="Float" + metric)


# ------------------------------------------------------------------------------------------
# the restart after a visited-list overflow, with partitions in lock-step and with a hub
# ------------------------------------------------------------------------------------------
def test_restart_inside_a_tree(wa, gpu, tmp_path, monkeypatch, capfd):
    n, d = 6000, 32
    X = sift_like(n, d, 82)(n)
    monkeypatch.setenv("WANN_BUILD_VIS_CAP", "64")
    monkeypatch.setenv("WANN_VERBOSE", "1")
    gf = _gpu_and_host(wa, monkeypatch, tmp_path, TREE, "FloatEuclidian", X, distinct_labels(n, 18), 24, 48, 1.0,
                       dict(cutoff=500, split_factor=2))
    assert len(gf) > 3
    assert capfd.readouterr().err.count("restarting the GPU build") >= 1


def test_restart_with_a_hub(oracle, wa, gpu, tmp_path, monkeypatch, capfd):
    n = 12000
    X = star_hub(n, 32, "mips", [int(oracle.random_permutation(n)[0])])
    monkeypatch.setenv("WANN_BUILD_VIS_CAP", "64")
    monkeypatch.setenv("WANN_VERBOSE", "1")
    _gpu_and_host(wa, monkeypatch, tmp_path, POST, "FloatMips", X, np.arange(n, dtype=np.float32), 16, 16, 1.0)
    err = capfd.readouterr().err
    assert err.count("restarting the GPU build") >= 1
    groups, rounds = _second_pass(err)
    assert groups > 0 and rounds >= 20


# ------------------------------------------------------------------------------------------
# degrees: one neighbour, one less than the wave width, the wave width
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 63, 64])
def test_degree_edges(wa, gpu, tmp_path, monkeypatch, R):
    n, d = 1500, 8
    X = sift_like(n, d, 83)(n)
    gf = _gpu_and_host(wa, monkeypatch, tmp_path, TREE, "FloatEuclidian", X, distinct_labels(n, 19), R, max(8, 2 * R), 1.2,
                       dict(cutoff=200, split_factor=2))
    for f, blob in gf.items():
        hdr = np.frombuffer(blob[:8], dtype=np.int32)
        deg = np.frombuffer(blob[8:8 + 4 * hdr[0]], dtype=np.int32)
        assert hdr[1] == R and 0 <= deg.min() and deg.max() <= R, f
