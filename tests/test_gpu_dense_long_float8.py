"""GPU: float8 rows of 129 .. 2048 elements on the dense paths (`k_gemm_scores_f8slab`), opted in per index with
`set_dense_long_float8(True)`; WANN_DENSE_LONG_ROWS is set for the float32 leg alone.  Batches, checks and caps: tests/test_gpu_dense_long_half.py's
on unit rows x 8 rounded to float8 (seeds checked with its score model: profiles/dense_long_float8_test_counters.txt)."""
import numpy as np
import pytest

import dense_long_half_inputs as half
import golden_util as gu
from test_gpu_dense_float8 import SCALE
from test_gpu_dense_long_half import _dense, _oracle_check, _scan_and_dense
from test_gpu_float8 import GRAPH_KINDS, SCAN_KINDS
from util import random_rows

pytestmark = pytest.mark.gpu
# 129: qw 144 in a 192-byte row, a last slab of one k-step ending in half a group; 160: the row ends mid-group; 256: two slabs;
# 513: a last slab of one k-step; 1000: of 112 elements; 2048: the limit
CASES = [(d, "shared", k) for d in (129, 160, 256, 513, 1000, 2048) for k in ((10, 1, 16) if d == 1000 else (10,))] + [(129, "cover", 10), (2048, "cover", 10)]
SFX, CAP, _cache = ("Float8Euclidian", "Float8Mips"), half.F * half.REP // 10, {}
_unit = lambda wa, x: wa.float8_round((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32) * SCALE)  # noqa: E731
# the class of the float32 index on the upcast rows, and the name the oracle helpers of the float16 test go by
_f32 = lambda sfx: sfx.replace("BFloat16", "Float").replace("Float8", "Float")  # noqa: E731


def _index(wa, sfx, d, on):
    """half.Batch(d) with X and Q replaced by float8 values (one d at a time), and the PrefilterIndex of class sfx on it, switch set to `on`"""
    if _cache.get("d") != d:
        bt, rng = half.Batch(d), np.random.default_rng(8800 + d)
        bt.X = bt.X32 = _unit(wa, rng.standard_normal((half.N, d)))
        bt.Q = bt.Q32 = _unit(wa, rng.standard_normal((half.F * half.REP, d)))
        _cache.clear()
        _cache.update(d=d, bt=bt)
    if sfx not in _cache:
        _cache[sfx] = getattr(wa, "PrefilterIndex" + sfx)(_cache["bt"].X, _cache["bt"].labels)
    assert _cache[sfx].set_dense_long_float8(on) is (on and "Float8" in sfx)
    return _cache[sfx], _cache["bt"]


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d,path,k", CASES)
def test_long_rows(oracle, wa, gpu, monkeypatch, sfx, d, path, k):
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_DENSE_LONG_ROWS", "1")
    fi, bt = _index(wa, _f32(sfx), d, False)
    W = bt.windows(path)
    fids, fdists, fctr = _dense(fi, wa, path, bt.Q, W, k)
    print(f"[dense long float8] {sfx} d={d} {path} k={k}: float32 index on the upcast: {fctr}")
    assert fctr["queries"] == len(bt.Q) and fctr["unproven"] <= CAP, (sfx, d, path, fctr)  # (the input's condition, on existing code)
    ids, dists, ctr = _scan_and_dense(_index(wa, sfx, d, True)[0], wa, monkeypatch, path, bt.Q, W, k, long_rows=False)
    print(f"[dense long float8] {sfx} d={d} {path} k={k}: {ctr}")
    _oracle_check(oracle, bt, _f32(sfx), path, k, ids, dists)
    assert ctr["queries"] == len(bt.Q) and ctr["unproven"] <= CAP, (sfx, d, path, ctr)
    assert np.array_equal(fids, ids) and np.array_equal(fdists.view(np.uint32), dists.view(np.uint32)), (sfx, d, path, k)
    assert d < 513 or fctr == ctr, (ctr, fctr)  # (k_gemm_scores_long: the same arithmetic on the same bits)


@pytest.mark.parametrize("sfx,d,want", [(s, d, w) for s in SFX for d, w in ((2049, 0), (100, 240))] + [("BFloat16Euclidian", 256, 0)])
def test_what_the_switch_does_not_move(oracle, wa, gpu, monkeypatch, sfx, d, want):
    """d = 2049: the scan; d = 100: the narrow kernel, the same counters on and off; a bfloat16 index refuses the switch (scan at d = 256)"""
    ctrs = []
    for on in (True, False):
        pi, bt = _index(wa, sfx, d, on)
        ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, "shared", bt.Q, bt.windows("shared"), 10, long_rows=False)
        _oracle_check(oracle, bt, _f32(sfx), "shared", 10, ids, dists)
        ctrs.append(ctr)
    assert ctrs[0] == ctrs[1] and ctrs[0]["queries"] == want and ctrs[0]["unproven"] <= want // 10, ctrs


@pytest.mark.parametrize("kind,kw", GRAPH_KINDS + SCAN_KINDS)
def test_return_values_and_defaults(wa, gpu, tmp_path, kind, kw):
    rng = np.random.default_rng(3)
    kw = dict(kw, build_params=wa.BuildParams(16, 32, 1.0, str(tmp_path) + "/")) if (kind, kw) in GRAPH_KINDS else kw
    for sfx in SFX + ("FloatEuclidian", "UInt8Euclidian", "Int8Mips", "Float16Mips", "BFloat16Euclidian"):
        idx = getattr(wa, kind + sfx)(random_rows(sfx, rng, 600, 20), rng.permutation(600).astype(np.float32), **kw)
        for ask, want in ((None, False), (True, "Float8" in sfx), (False, False)):
            assert ask is None or idx.set_dense_long_float8(ask) is want
            assert idx.dense_long_float8() is want and idx.counters()["dense_long_float8"] == int(want), (kind, sfx, ask)


def test_tree_exact_windows(wa, gpu, monkeypatch, tmp_path):
    """test_gpu_dense_long_half.py's sorted-exact shape: 64 windows of 1 100 .. 2 900 positions over position blocks 0 and 1"""
    d, n, k, L, nq, B = 768, 6000, 10, 3000, 64, half.BLOCK
    rng = np.random.default_rng(8768)
    X, Q, labels = _unit(wa, rng.standard_normal((n, d))), _unit(wa, rng.standard_normal((nq, d))), rng.permutation(n).astype(np.float32)
    a = rng.integers(1000, 1901, nq)
    W = np.stack([a - 0.5, a + np.array([rng.integers(max(1100, B + 1 - s), min(2900, 2 * B - s) + 1) for s in a]) - 0.5], 1)
    idx = wa.VamanaRangeFilterTreeIndexFloat8Euclidian(X, labels, cutoff=500, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/"))
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    assert idx.set_dense_long_float8(True) is True and idx.set_exact_windows(L) == 0
    (i0, d0), e0 = idx.batch_search(Q, W, nq, "optimized_postfilter", half.qp(wa, k)), idx.exact_window_counters()
    pids, pd = wa.PrefilterIndexFloat8Euclidian(X, labels).batch_search(Q, W, nq, half.qp(wa, k))  # the exact rows
    monkeypatch.delenv("WANN_NO_GEMM")
    (i1, d1), e1 = idx.batch_search(Q, W, nq, "optimized_postfilter", half.qp(wa, k)), idx.exact_window_counters()
    print(f"[dense long float8] tree d={d} exact windows L={L}: {e1}")
    assert e0["queries"] == nq and e0["dense_queries"] == 0 and e0["passes"] == 0, e0
    assert e1["queries"] == nq and e1["dense_queries"] == nq and e1["unproven"] <= nq // 10, e1
    assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    ok, why = gu.same_rows(pids, pd, i1, d1, True, gu.RowContext(X, labels, Q, W, "l2", "prefilter"))
    assert ok, why
