"""GPU: k = 17 .. 128 on the dense paths (`k_large_rerank` / `k_large_rerank_cover`), opted in per index with
`set_dense_large_k(True)`.  Random unit rows, n = 14 000, 48 queries; a window holds exactly 96 k positions (the gate) unless a
case says otherwise.  Per case: under WANN_NO_GEMM the exact scan alone, then the dense path -- the same ids and distance bits --
and the scan's rows against the float32 oracle; every query counted on its path, at most a tenth of the batch unproven."""
import numpy as np
import pytest

import dense_long_half_inputs as half
import golden_util as gu
from test_gpu_dense_long_half import _dense, _oracle_check, _scan_and_dense
from test_gpu_float8 import GRAPH_KINDS, SCAN_KINDS
from util import pos_windows, random_rows

pytestmark = pytest.mark.gpu
N, NQ, GATE, NONE, _cache = 14000, 48, 96, dict(queries=0, unproven=0, rescued=0), {}
# 17: first k past the lane list; 33: past kSelect; 64: more than one wave_distances pass; 100; 128: the limit
ROWS = [(sfx, 24, path, k) for k in (17, 33, 64, 100, 128) for sfx in ("FloatEuclidian", "FloatMips") for path in ("shared", "cover")]
ROWS += [("FloatEuclidian", 160, "shared", 100), ("Float8Euclidian", 24, "shared", 100)]  # the wide row class; another unit


class _Batch:
    """rows, queries, labels (a permutation: positions are labels) and the index of class sfx; `W` is the case's windows"""

    def __init__(self, wa, sfx, d):
        rng = np.random.default_rng(1700 + d)
        rows = (lambda m: wa.float8_round(random_rows("Float", rng, m, d) * 8)) if "Float8" in sfx else (lambda m: random_rows(sfx, rng, m, d))
        self.d, self.X32, self.Q32, self.labels = d, rows(N), rows(NQ), rng.permutation(N).astype(np.float32)
        self.index, self.W = getattr(wa, "PrefilterIndex" + sfx)(self.X32, self.labels), None

    def windows(self, path):
        return self.W

    def oracle_rows(self, oracle, sfx, path, k):
        return getattr(oracle, "PrefilterIndex" + sfx)(self.X32, self.labels).batch_search(self.Q32, self.W, NQ, half.qp(oracle, k))


def _windows(path, w):
    """shared: three groups of 16 queries (kGroupMinQueries) on [a, a + w), one a on a 128-position step, two off it; cover: 48
    distinct windows [300 + j, 300 + j + w) whose ends all lie in one position block, so every block has 48 >= 32 wide queries"""
    a = np.repeat([0, 129, 333], NQ // 3) if path == "shared" else 300 + np.arange(NQ)
    assert a.max() + w <= N - 64 and (path == "shared" or (299 + w) // half.BLOCK == (346 + w) // half.BLOCK)
    return pos_windows(a, a + w)


def _run(oracle, wa, monkeypatch, sfx, d, path, k, w, on=True):
    if (sfx, d) not in _cache:
        _cache[sfx, d] = _Batch(wa, sfx, d)
    bt = _cache[sfx, d]
    bt.W = _windows(path, w)
    assert bt.index.set_dense_large_k(on) is (on and "Int8" not in sfx) and bt.index.counters()["dense_large_k"] == int(bt.index.dense_large_k())
    ids, dists, ctr = _scan_and_dense(bt.index, wa, monkeypatch, path, bt.Q32, bt.W, k, long_rows=False)
    print(f"[dense large k] {sfx} d={d} {path} k={k} w={w} switch={on}: {ctr}")
    if "Int8" not in sfx:
        _oracle_check(oracle, bt, sfx.replace("Float8", "Float"), path, k, ids, dists)
    return ids, dists, ctr


@pytest.mark.parametrize("sfx,d,path,k", ROWS)
def test_rows(oracle, wa, gpu, monkeypatch, sfx, d, path, k):
    ctr = _run(oracle, wa, monkeypatch, sfx, d, path, k, GATE * k)[2]
    assert ctr["queries"] == NQ and ctr["unproven"] <= NQ // 10, ctr


@pytest.mark.parametrize("k,w", [(17, 5440), (17, 5504), (100, 12000)])
def test_pending_buffer_edges(oracle, wa, gpu, monkeypatch, k, w):
    """85 / 86 blocks of three candidates: 255 (the list never fills) and 258 (two dropped); 188 blocks: three trips, several merges"""
    ctr = _run(oracle, wa, monkeypatch, "FloatEuclidian", 24, "shared", k, w)[2]
    assert ctr["queries"] == NQ and ctr["unproven"] <= NQ // 10, ctr


@pytest.mark.parametrize("sfx,k,w,on", [("FloatEuclidian", 17, GATE * 17 - 1, True), ("FloatEuclidian", 129, GATE * 129, True),
                                        ("FloatEuclidian", 100, GATE * 100, False), ("UInt8Euclidian", 100, GATE * 100, True)])
@pytest.mark.parametrize("path", ("shared", "cover"))
def test_gate_and_limits(oracle, wa, gpu, monkeypatch, path, sfx, k, w, on):
    """a window one position under the gate, k past the limit, the switch off, a byte index (which refuses it): the scan's rows"""
    assert _run(oracle, wa, monkeypatch, sfx, 24, path, k, w, on)[2] == NONE


def test_k10_does_not_see_the_switch(oracle, wa, gpu, monkeypatch):
    on, off = (_run(oracle, wa, monkeypatch, "FloatEuclidian", 24, "shared", 10, 1024, s) for s in (True, False))
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1].view(np.uint32), off[1].view(np.uint32)) and on[2] == off[2] and on[2]["queries"] == NQ


def test_tree_exact_windows(wa, gpu, monkeypatch, tmp_path):
    """tests/test_gpu_dense_long_half.py's sorted-exact shape at k = 64: 64 windows of 6 150 .. 7 000 positions (>= 96 k) from block 0 to block 3"""
    d, n, k, L, nq = 24, 9000, 64, 7100, 64
    rng = np.random.default_rng(1764)
    X, Q, labels = random_rows("Float", rng, n, d), random_rows("Float", rng, nq, d), rng.permutation(n).astype(np.float32)
    a = rng.integers(1000, 1048, nq)
    W = pos_windows(a, a + rng.integers(GATE * k + 6, 7001 - 48, nq))
    idx = wa.VamanaRangeFilterTreeIndexFloatEuclidian(X, labels, cutoff=500, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/"))
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    assert idx.set_dense_large_k(True) is True and idx.set_exact_windows(L) == 0
    (i0, d0), e0 = idx.batch_search(Q, W, nq, "optimized_postfilter", half.qp(wa, k)), idx.exact_window_counters()
    pids, pd = wa.PrefilterIndexFloatEuclidian(X, labels).batch_search(Q, W, nq, half.qp(wa, k))  # the exact rows
    monkeypatch.delenv("WANN_NO_GEMM")
    (i1, d1), e1 = idx.batch_search(Q, W, nq, "optimized_postfilter", half.qp(wa, k)), idx.exact_window_counters()
    print(f"[dense large k] tree k={k} exact windows L={L}: {e1}")
    assert e0["queries"] == nq and e0["dense_queries"] == 0 and e0["passes"] == 0, e0
    assert e1["queries"] == nq and e1["dense_queries"] == nq and e1["unproven"] <= nq // 10, e1
    assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    ok, why = gu.same_rows(pids, pd, i1, d1, True, gu.RowContext(X, labels, Q, W, "l2", "prefilter"))
    assert ok, why


@pytest.mark.parametrize("kind,kw", GRAPH_KINDS + SCAN_KINDS)
def test_return_values_and_defaults(wa, gpu, tmp_path, kind, kw):
    rng = np.random.default_rng(3)
    kw = dict(kw, build_params=wa.BuildParams(16, 32, 1.0, str(tmp_path) + "/")) if (kind, kw) in GRAPH_KINDS else kw
    for sfx in ("FloatEuclidian", "UInt8Euclidian", "Int8Mips", "Float16Mips", "BFloat16Euclidian", "Float8Mips"):
        idx = getattr(wa, kind + sfx)(random_rows(sfx, rng, 600, 20), rng.permutation(600).astype(np.float32), **kw)
        for ask, want in ((None, False), (True, "Int8" not in sfx), (False, False)):
            assert ask is None or idx.set_dense_large_k(ask) is want
            assert idx.dense_large_k() is want and idx.counters()["dense_large_k"] == int(want), (kind, sfx, ask)
