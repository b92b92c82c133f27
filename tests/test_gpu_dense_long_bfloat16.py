"""GPU: bfloat16 rows of 129 .. 2048 elements on the dense paths (`k_gemm_scores_bfslab`), opted in per index with
`set_dense_long_rows(True)`; WANN_DENSE_LONG_ROWS is set for the float32 leg alone.  Batches, checks and caps are those of
tests/test_gpu_dense_long_half.py on rows rounded to bfloat16 (seeds checked with its score model: profiles/dense_long_bfloat16_test_counters.txt)."""
import numpy as np
import pytest

import dense_long_half_inputs as half
import golden_util as gu
from test_gpu_dense_long_half import _dense, _oracle_check, _scan_and_dense
from test_gpu_float8 import GRAPH_KINDS, SCAN_KINDS
from util import random_rows

pytestmark = pytest.mark.gpu
# 129: qw 144 but 160 elements a row; 160: the two agree; 256: two slabs; 513: a last slab of one k-step; 1000: of 112; 2048: the limit
CASES = [(d, "shared", k) for d in (129, 160, 256, 513, 1000, 2048) for k in ((10, 1, 16) if d == 1000 else (10,))] + [(129, "cover", 10), (2048, "cover", 10)]
SFX = ("BFloat16Euclidian", "BFloat16Mips")
_cache = {}


def _unit(wa, x):
    return wa.bfloat16_round((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


class Batch(half.Batch):
    """half.Batch's labels, families and windows; X and Q are float32 arrays of bfloat16 values"""

    def __init__(self, wa, d):
        super().__init__(d)
        rng = np.random.default_rng(7500 + d)
        self.X = self.X32 = _unit(wa, rng.standard_normal((half.N, d)))
        self.Q = self.Q32 = _unit(wa, rng.standard_normal((half.F * half.REP, d)))

    def oracle_rows(self, oracle, sfx, path, k):
        return super().oracle_rows(oracle, sfx.replace("BFloat16", "Float16"), path, k)  # (half's rule for the Float class name)


def _index(wa, sfx, d, on):
    """the batch of row length d (one at a time) and the PrefilterIndex of class sfx on it, the switch set to `on`"""
    if _cache.get("d") != d:
        _cache.clear()
        _cache.update(d=d, bt=Batch(wa, d))
    if sfx not in _cache:
        _cache[sfx] = getattr(wa, "PrefilterIndex" + sfx)(_cache["bt"].X, _cache["bt"].labels)
    assert _cache[sfx].set_dense_long_rows(on) is (on and "BFloat16" in sfx)
    return _cache[sfx], _cache["bt"]


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d,path,k", CASES)
def test_long_rows(oracle, wa, gpu, monkeypatch, sfx, d, path, k):
    pi, bt = _index(wa, sfx, d, True)
    W = bt.windows(path)
    ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, path, bt.Q, W, k, long_rows=False)
    _oracle_check(oracle, bt, sfx, path, k, ids, dists)
    monkeypatch.setenv("WANN_DENSE_LONG_ROWS", "1")
    fids, fdists, fctr = _dense(_index(wa, sfx.replace("BFloat16", "Float"), d, False)[0], wa, path, bt.Q, W, k)
    print(f"[dense long bfloat16] {sfx} d={d} {path} k={k}: {ctr}; float32 index on the upcast: {fctr}")
    assert ctr["queries"] == len(bt.Q) and ctr["unproven"] <= len(bt.Q) // 10, (sfx, d, path, ctr)
    assert np.array_equal(fids, ids) and np.array_equal(fdists.view(np.uint32), dists.view(np.uint32)), (sfx, d, path, k)
    assert d < 513 or fctr == ctr, (ctr, fctr)  # (k_gemm_scores_long: the same arithmetic on the same bits)


@pytest.mark.parametrize("sfx,d,on,want", [(s, d, on, w) for s in SFX for d, on, w in ((2049, True, 0), (100, True, 240), (100, False, 240))]
                         + [("Float16Euclidian", 256, True, 0)])
def test_what_the_switch_does_not_move(oracle, wa, gpu, monkeypatch, sfx, d, on, want):
    """d = 2049: the scan; d = 100, on and off: the narrow kernel; a float16 index refuses the switch and keeps d = 256 on the scan"""
    pi, bt = _index(wa, sfx, d, on)
    ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, "shared", bt.Q, bt.windows("shared"), 10, long_rows=False)
    assert ctr == dict(queries=want, unproven=0, rescued=0), ctr
    if "BFloat16" in sfx:  # (the float16 index rounds these rows once more: its own scan is its check)
        _oracle_check(oracle, bt, sfx, "shared", 10, ids, dists)


@pytest.mark.parametrize("kind,kw", GRAPH_KINDS + SCAN_KINDS)
def test_return_values_and_defaults(wa, gpu, tmp_path, kind, kw):
    rng = np.random.default_rng(3)
    labels = rng.permutation(600).astype(np.float32)
    if (kind, kw) in GRAPH_KINDS:
        kw = dict(kw, build_params=wa.BuildParams(16, 32, 1.0, str(tmp_path) + "/"))
    for sfx in SFX + ("FloatEuclidian", "UInt8Euclidian", "Int8Mips", "Float16Mips", "Float8Euclidian"):
        idx = getattr(wa, kind + sfx)(random_rows(sfx, rng, 600, 20), labels, **kw)
        for ask, want in ((None, False), (True, "BFloat16" in sfx), (False, False)):
            assert ask is None or idx.set_dense_long_rows(ask) is want
            assert idx.dense_long_rows() is want and idx.counters()["dense_long_rows"] == int(want), (kind, sfx, ask)


def test_tree_exact_windows(wa, gpu, monkeypatch, tmp_path):
    """test_gpu_dense_long_half.py's sorted-exact shape: 64 windows of 1 100 .. 2 900 positions over position blocks 0 and 1"""
    d, n, k, L, nq, B = 768, 6000, 10, 3000, 64, half.BLOCK
    rng = np.random.default_rng(7768)
    X, Q = _unit(wa, rng.standard_normal((n, d))), _unit(wa, rng.standard_normal((nq, d)))
    labels = rng.permutation(n).astype(np.float32)
    a = rng.integers(1000, 1901, nq)
    w = np.array([rng.integers(max(1100, B + 1 - s), min(2900, 2 * B - s) + 1) for s in a])
    W = np.stack([a - 0.5, a + w - 0.5], 1)
    idx = wa.VamanaRangeFilterTreeIndexBFloat16Euclidian(X, labels, cutoff=500, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/"))
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    assert idx.set_dense_long_rows(True) is True and idx.set_exact_windows(L) == 0
    i0, d0 = idx.batch_search(Q, W, nq, "optimized_postfilter", half.qp(wa, k))
    e0 = idx.exact_window_counters()
    pids, pd = wa.PrefilterIndexBFloat16Euclidian(X, labels).batch_search(Q, W, nq, half.qp(wa, k))  # the exact rows
    monkeypatch.delenv("WANN_NO_GEMM")
    i1, d1 = idx.batch_search(Q, W, nq, "optimized_postfilter", half.qp(wa, k))
    e1 = idx.exact_window_counters()
    print(f"[dense long bfloat16] tree d={d} exact windows L={L}: {e1}")
    assert e0["queries"] == nq and e0["dense_queries"] == 0 and e0["passes"] == 0, e0
    assert e1["queries"] == nq and e1["dense_queries"] == nq and e1["unproven"] <= nq // 10, e1
    assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    ok, why = gu.same_rows(pids, pd, i1, d1, True, gu.RowContext(X, labels, Q, W, "l2", "prefilter"))
    assert ok, why
