"""GPU: k = 17 .. 128 on the dense paths of uint8 / int8 indexes (`k_large_rerank_b` / `k_large_rerank_cover_b`), opted in per
index with `set_dense_large_k_bytes(True)`.  n = 14 000, 48 queries, labels a permutation, windows of exactly 96 k positions (the
gate) unless a case says otherwise.  Per case: the exact scan under WANN_NO_GEMM, then the dense path -- the same ids and distance
bits --, the scan's rows against an int64 brute force over the window ordered by (distance, id), and the path's counters.  Rows
of up to 512 bytes return the distances their selection keys hold, so the tie inputs (few distinct values: most queries tie at
the k-th distance) are what the re-ordering from (distance, position) to (distance, id) has to get right."""
import numpy as np
import pytest

import golden_util as gu
from dense_long_half_inputs import qp
from test_gpu_dense_large_k import GATE, N, NONE, NQ, _windows
from test_gpu_dense_long_half import _scan_and_dense
from util import pos_windows, random_rows

pytestmark = pytest.mark.gpu
_cache = {}
# class, d, rows(rng, m): few distinct values; "iz": rows <= 0 and queries >= 0 with 8 non-zero entries, so a query's best inner
# products are some 37 zeros -- which the scan returns as -0.0
TIES = {"u16": ("UInt8Euclidian", 24, lambda r, m: r.integers(0, 16, (m, 24))), "u4": ("UInt8Euclidian", 8, lambda r, m: r.integers(0, 4, (m, 8))),
        "i16": ("Int8Mips", 24, lambda r, m: r.integers(-8, 8, (m, 24))),
        "iz": ("Int8Mips", 24, lambda r, m: r.integers(1, 100, (m, 24)) * r.permuted(np.tile(np.arange(24) < 8, (m, 1)), axis=1) if m == NQ
                                  else -r.integers(1, 100, (m, 24)) * (r.random((m, 24)) < 0.5))}
# 17: first k past the lane list; 33: past kSelect; 64, 100: more than one merge pass; 128: the limit
CASES = [(sfx, 24, path, k, GATE * k) for k in (17, 33, 64, 100, 128) for sfx in ("UInt8Euclidian", "Int8Mips") for path in ("shared", "cover")]
CASES += [("UInt8Mips", 24, "shared", 100, 9600), ("Int8Euclidian", 24, "shared", 100, 9600)]  # the other bias / offset formulas
CASES += [("UInt8Mips", 512, "shared", 100, 9600)]  # the largest key offset of the unquantised keys: sums beyond 2^24
CASES += [("UInt8Euclidian", 600, "shared", 100, 9600), ("Int8Mips", 600, "shared", 100, 9600)]  # quantised keys (WANN_DENSE_LONG_ROWS=1)
CASES += [(t, 0, path, 100, 9600) for t in TIES for path in ("shared", "cover")]
# 85 / 86 blocks of three candidates: 255 (the list never fills) and 258 (two dropped); 188 blocks: three trips
CASES += [("UInt8Euclidian", 24, "shared", 17, 64 * b) for b in (85, 86, 188)]


def _batch(wa, name, d):
    """(index, rows, queries, label order) of class `name` / a TIES input, cached"""
    if (name, d) not in _cache:
        rng = np.random.default_rng(1900 + d + sum(map(ord, name)))
        sfx, dd, gen = TIES.get(name, (name, d, None))
        rows = (lambda m: random_rows(sfx, rng, m, dd)) if gen is None else (lambda m: gen(rng, m).astype(np.int8 if "Int8" == sfx[:4] else np.uint8))
        X, Q, labels = rows(N), rows(NQ), rng.permutation(N).astype(np.float32)
        _cache[name, d] = (getattr(wa, "PrefilterIndex" + sfx)(X, labels), X, Q, np.argsort(labels), sfx)
    return _cache[name, d]


def _brute(X, Q, order, W, k, mips):
    """the window's rows by (exact integer distance, id): ids and the distances as float32"""
    ids, dists = np.empty((len(Q), k), np.int64), np.empty((len(Q), k), np.float32)
    for i, (q, (a, b)) in enumerate(zip(Q.astype(np.int64), np.ceil(W).astype(np.int64))):
        rows = np.sort(order[a:b])
        x = X[rows].astype(np.int64)
        s = x @ q if mips else ((x - q) ** 2).sum(1)
        top = np.lexsort((rows, -s if mips else s))[:k]
        ids[i], dists[i] = rows[top], -s[top].astype(np.float32) if mips else s[top]  # (the scan negates after the cast: a zero inner product is -0.0)
    return ids, dists


def _run(wa, monkeypatch, name, d, path, k, w, on=True, Q=None):
    idx, X, Q0, order, sfx = _batch(wa, name, d)
    W = _windows(path, w)
    assert idx.set_dense_large_k(True) is False and idx.set_dense_large_k_bytes(on) is on and idx.counters()["dense_large_k_bytes"] == int(on)
    ids, dists, ctr = _scan_and_dense(idx, wa, monkeypatch, path, Q0 if Q is None else Q, W, k, long_rows=X.shape[1] > 512)
    print(f"[dense large k bytes] {name} d={X.shape[1]} {path} k={k} w={w} switch={on}: {ctr}")
    if Q is None:
        bi, bd = _brute(X, Q0, order, W, k, sfx.endswith("Mips"))
        assert np.array_equal(ids, bi) and np.array_equal(dists.view(np.uint32), bd.view(np.uint32)), (name, path, k)
    return ctr


@pytest.mark.parametrize("name,d,path,k,w", CASES)
def test_rows(wa, gpu, monkeypatch, name, d, path, k, w):
    ctr = _run(wa, monkeypatch, name, d, path, k, w)
    assert ctr["queries"] == NQ and ctr["unproven"] <= NQ // 10, ctr


def test_float_queries_pack_by_one_rule(wa, gpu, monkeypatch):
    """fractional and out-of-range float32 queries on a uint8 index: the scan and the dense path see the same bytes"""
    Q = _batch(wa, "UInt8Euclidian", 24)[1][100:100 + NQ].astype(np.float32) + 0.4
    Q[::3, 5], Q[1::3, 7] = -5.0, 300.0
    ctr = _run(wa, monkeypatch, "UInt8Euclidian", 24, "shared", 100, 9600, Q=Q)
    assert ctr["queries"] == NQ and ctr["unproven"] <= NQ // 10, ctr


@pytest.mark.parametrize("k,w,on", [(100, 9600, False), (129, GATE * 129, True), (17, GATE * 17 - 1, True)])
@pytest.mark.parametrize("path", ("shared", "cover"))
def test_gate_and_limits(wa, gpu, monkeypatch, path, k, w, on):
    """the switch off, k past the limit, a window one position under the gate: the scan's rows, no dense query"""
    assert _run(wa, monkeypatch, "UInt8Euclidian", 24, path, k, w, on) == NONE
    f = wa.PrefilterIndexFloatEuclidian(np.eye(4, dtype=np.float32), np.arange(4, dtype=np.float32))
    assert f.set_dense_large_k_bytes(True) is False and f.dense_large_k_bytes() is False and f.counters()["dense_large_k_bytes"] == 0


def test_tree_exact_windows(wa, gpu, monkeypatch, tmp_path):
    """tests/test_gpu_dense_large_k.py's sorted-exact shape at k = 100: 64 windows of 9 606 .. 10 450 positions (>= 96 k)"""
    d, k, L, nq = 24, 100, 10600, 64
    rng = np.random.default_rng(1964)
    X, Q, labels = random_rows("UInt8", rng, N, d), random_rows("UInt8", rng, nq, d), rng.permutation(N).astype(np.float32)
    a = rng.integers(1000, 1048, nq)
    W = pos_windows(a, a + rng.integers(GATE * k + 6, 10501 - 48, nq))
    idx = wa.VamanaRangeFilterTreeIndexUInt8Euclidian(X, labels, cutoff=500, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/"))
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    assert idx.set_dense_large_k_bytes(True) is True and idx.set_exact_windows(L) == 0
    (i0, d0), e0 = idx.batch_search(Q, W, nq, "optimized_postfilter", qp(wa, k)), idx.exact_window_counters()
    monkeypatch.delenv("WANN_NO_GEMM")
    (i1, d1), e1 = idx.batch_search(Q, W, nq, "optimized_postfilter", qp(wa, k)), idx.exact_window_counters()
    print(f"[dense large k bytes] tree k={k} exact windows L={L}: {e1}")
    assert e0["queries"] == nq and e0["dense_queries"] == 0 and e0["passes"] == 0, e0
    assert e1["queries"] == nq and e1["dense_queries"] == nq and e1["unproven"] <= nq // 10, e1
    assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    bi, bd = _brute(X, Q, np.argsort(labels), W, k, False)
    ok, why = gu.same_rows(bi.astype(i1.dtype), bd, i1, d1, True, gu.RowContext(X, labels, Q, W, "l2", "prefilter"))
    assert ok, why
