"""GPU: the dense (MFMA) prefilter path on uint8, int8 and float16 point sets.

Shared-window PrefilterIndex batches of these element types run on the matrix cores like float32 ones: byte rows on the int8
MFMA with exact int32 scores, float16 rows on the bf16 kernels with half loads.  The contract is the float32 path's: a batch
returns exactly the rows (ids and distance bits) of the exact scan (WANN_NO_GEMM=1), whatever the dense path cannot settle is
counted in gemm_unproven -- and on well-spread data that must stay a small share, or a path that settles nothing would pass
every row test."""
import numpy as np
import pytest

import golden_util as gu
from util import clustered_window_batch, repeated_labels, sift_like

pytestmark = pytest.mark.gpu

BYTE_CLASSES = ("UInt8Euclidian", "UInt8Mips", "Int8Euclidian", "Int8Mips")
HALF_CLASSES = ("Float16Euclidian", "Float16Mips")


def _qp(mod, k=10):
    return mod.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def _elem(sfx):
    return np.uint8 if sfx.startswith("UInt8") else np.int8 if sfx.startswith("Int8") else np.float16


def _quantise(sfx, x):
    """unit-scale floats as the class of suffix sfx stores them: round(127 x) for int8, + 128 for uint8, binary16 otherwise"""
    if sfx.startswith("Float16"):
        return x.astype(np.float16)
    q = np.rint(127.0 * np.clip(x, -1, 1))
    return (q + 128).astype(np.uint8) if sfx.startswith("UInt8") else q.astype(np.int8)


def _random_rows(sfx, rng, n, d):
    """well-spread rows: uniform random bytes, unit vectors for float16"""
    if sfx.startswith("UInt8"):
        return rng.integers(0, 256, (n, d)).astype(np.uint8)
    if sfx.startswith("Int8"):
        return rng.integers(-128, 128, (n, d)).astype(np.int8)
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)


def _oracle_index(oracle, sfx, X, labels):
    """the oracle's PrefilterIndex for the class of suffix sfx and what it takes as queries: float16 classes are checked against
    the float32 oracle on the exact upcast, which is what a float16 index promises to return"""
    if sfx.startswith("Float16"):
        return getattr(oracle, "PrefilterIndex" + sfx.replace("Float16", "Float"))(X.astype(np.float32), labels), np.float32
    return getattr(oracle, "PrefilterIndex" + sfx)(X, labels), X.dtype


def _both_paths(pi, wa, monkeypatch, Q, W, k):
    """one batch on the dense path and on the exact scan: (ids, dists, counters of the dense run); the rows must be equal"""
    nq = len(Q)
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    ids, dists = pi.batch_search(Q, W, nq, _qp(wa, k))
    c = pi.counters()
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    ids2, dists2 = pi.batch_search(Q, W, nq, _qp(wa, k))
    assert pi.counters()["gemm_queries"] == 0
    monkeypatch.delenv("WANN_NO_GEMM")
    assert np.array_equal(dists.view(np.uint32), dists2.view(np.uint32)), (k, int((dists != dists2).any(axis=1).sum()), c)
    assert np.array_equal(ids, ids2), (k, int((ids != ids2).any(axis=1).sum()), c)
    return ids, dists, c


def typed_dense_batch(sfx):
    """X, Q, labels, W of test_typed_dense_prefilter_matches_oracle in the element type of the class of suffix sfx: the float32
    test's construction (util.clustered_window_batch), quantised"""
    if sfx.endswith("Euclidian"):
        X, Q, labels, W = clustered_window_batch(128, "sift")  # integers in [0, 255]
        if sfx.startswith("Int8"):
            X, Q = X - 128, Q - 128
        X, Q = X.astype(_elem(sfx)), Q.astype(_elem(sfx))
    else:
        X, Q, labels, W = clustered_window_batch(100, "unit")
        # (int8 / uint8: scaled so that the largest elements reach the ends of the byte range)
        s = 1.0 if sfx.startswith("Float16") else 3.0
        X = _quantise(sfx, s * X / np.linalg.norm(X, axis=1, keepdims=True))
        Q = _quantise(sfx, s * Q / np.linalg.norm(Q, axis=1, keepdims=True))
    return np.ascontiguousarray(X), Q, labels, W


@pytest.mark.parametrize("sfx", BYTE_CLASSES + HALF_CLASSES)
def test_typed_dense_prefilter_matches_oracle(oracle, wa, gpu, monkeypatch, sfx):
    """Clustered labels = clustered geometry, 40 queries per cluster window (the construction of the float32 test, quantised):
    most of the batch runs on the matrix cores, and its rows are the exact scan's, the oracle's, and -- for float16 -- the
    float32 index's on the upcast points."""
    X, Q, labels, W = typed_dense_batch(sfx)
    nq = Q.shape[0]
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    oi, oq = _oracle_index(oracle, sfx, X, labels)
    ctx = gu.RowContext(X.astype(np.float32), labels, Q.astype(np.float32), W, gu.metric_of(sfx), "prefilter")
    f32 = getattr(wa, "PrefilterIndex" + sfx.replace("Float16", "Float"))(X.astype(np.float32), labels) if sfx in HALF_CLASSES else None
    for k in (1, 10, 16):
        ids, dists, c = _both_paths(pi, wa, monkeypatch, Q, W, k)
        print(f"[typed dense] {sfx} k={k}: {c['gemm_queries']} of {nq} dense, unproven {c['gemm_unproven']}, rescued {c['gemm_rescued']}")
        assert c["gemm_queries"] > nq // 2, c
        eids, edists = oi.batch_search(Q.astype(oq), W, nq, _qp(oracle, k))
        ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
        assert ok, f"{sfx} k={k}: {why}"
        if f32 is not None:
            fids, fdists = f32.batch_search(Q.astype(np.float32), W, nq, _qp(wa, k))
            assert f32.counters()["gemm_queries"] == c["gemm_queries"]
            assert np.array_equal(fids, ids) and np.array_equal(fdists.view(np.uint32), dists.view(np.uint32)), k


def _families(nq=700):
    W = np.zeros((nq, 2))
    W[:300] = (100.5, 25100.5)       # 25 000 positions: eight slices of 3 200; three query tiles
    W[300:520] = (30000.5, 35000.5)  # 5 000 positions: three slices; two tiles
    W[520:560] = (-1, 1e9)           # everything
    W[560:660] = (500.5, 1800.5)     # 1 300 positions: one short slice
    W[660:] = (7.5, 250.5)           # below the minimum window: exact scan
    return W


SLICE_CASES = [(s, d, "random") for s in BYTE_CLASSES for d in (20, 64, 100, 128, 512)] + \
              [(s, d, "random") for s in HALF_CLASSES for d in (24, 100, 128)] + \
              [("UInt8Euclidian", 64, "drift"), ("UInt8Mips", 20, "drift"), ("Int8Mips", 100, "drift"), ("Int8Euclidian", 512, "drift"),
               ("Float16Mips", 24, "drift")]


@pytest.mark.parametrize("sfx,d,style", SLICE_CASES)
def test_typed_dense_prefilter_slices_and_tiles(wa, gpu, monkeypatch, sfx, d, style):
    """The window families of the float32 test (several slices, several query tiles, the whole index, one short slice, one
    family below the minimum window), a block of duplicated rows, every row length class of the score kernels; "drift": labels
    that follow the first query's score, so that a query's best points sit side by side in the window and defeat the per-lane
    hand-over -- those blocks are re-scanned exactly (gemm_rescued).  Rows equal the exact scan's; on well-spread rows of 64
    elements or more at k = 10 fewer than 10 % of the dense queries may go back to the exact scan (the float32 test's cap: 66 of 660)."""
    rng = np.random.default_rng(5)
    n, nq = 42000, 700
    X = _random_rows(sfx, rng, n, d)
    Q = _random_rows(sfx, rng, nq, d)
    X[1000:1040] = X[1000]  # duplicates
    labels = rng.permutation(n).astype(np.float32)
    if style == "drift":  # sorted by the score of the first query: later labels = better candidates
        x, q0 = X.astype(np.float64), Q[0].astype(np.float64)
        score = x @ q0 if sfx.endswith("Mips") else -((x - q0) ** 2).sum(axis=1)
        labels = np.empty(n, dtype=np.float32)
        labels[np.argsort(score, kind="stable")] = np.arange(n, dtype=np.float32)
        if sfx.startswith("Float16"):
            Q = (Q[0].astype(np.float32) * (1 + 0.01 * rng.standard_normal((nq, 1)))).astype(np.float16)
        else:  # the first query with one element in eight moved by one step
            step = (rng.random((nq, d)) < 0.125) * rng.choice([-1, 1], (nq, d))
            lo, hi = (0, 255) if sfx.startswith("UInt8") else (-128, 127)
            Q = np.clip(Q[0].astype(np.int32) + step, lo, hi).astype(_elem(sfx))
    W = _families(nq)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    for k in (10, 1):
        ids, dists, c = _both_paths(pi, wa, monkeypatch, Q, W, k)
        print(f"[typed dense] {sfx} d={d} {style} k={k}: unproven {c['gemm_unproven']}, rescued {c['gemm_rescued']} of {c['gemm_queries']}")
        assert c["gemm_queries"] == 660, c
        # (float16: the float32 test's own capped case, unit vectors at d = 100 under the inner product)
        if style == "random" and k == 10 and (d >= 64 if sfx in BYTE_CLASSES else (sfx, d) == ("Float16Mips", 100)):
            assert c["gemm_unproven"] < 66, c
        if style == "drift" and k == 10:
            assert c["gemm_rescued"] > 0, c


def _shared_windows(labels, nq, seed):
    """windows shared by groups of 20 queries, each of 1 100 .. 6 000 points, ends from the sorted labels (inside runs of equal
    labels); every tenth query has a window of its own"""
    rng = np.random.default_rng(seed)
    s = np.sort(labels)
    n = len(s)
    W = np.zeros((nq, 2))
    for g0 in range(0, nq, 20):
        w = int(rng.integers(1100, 6000))
        st = int(rng.integers(0, n - w))
        W[g0:g0 + 20] = (s[st], s[st + w])
    W[-20:] = (s[-3000], s[-1])        # hi = the largest label
    W[-40:-20] = (s[0] - 1, s[2500])   # lo below the smallest label
    for i in range(5, nq, 10):
        st = int(rng.integers(0, n - 300))
        W[i] = (s[st], s[st + int(rng.integers(0, 300))])
    return W


@pytest.mark.parametrize("d", (4, 32))
@pytest.mark.parametrize("sfx", BYTE_CLASSES)
def test_typed_dense_prefilter_ties(oracle, wa, gpu, monkeypatch, sfx, d):
    """Three-valued elements and repeated labels: most queries have many points at their k-th distance, in and out of what the
    score kernel hands over.  The exact scan orders by (dist, id); a dense path that takes "no better than the bound" for
    "worse than the bound" returns a wrong id here.  Rows equal the exact scan's bit for bit and the oracle's up to its ties."""
    rng = np.random.default_rng(41 + d)
    n, nq = 20000, 400
    lo = 0 if sfx.startswith("UInt8") else -1
    X = rng.integers(lo, lo + 3, (n, d)).astype(_elem(sfx))
    Q = rng.integers(lo, lo + 3, (nq, d)).astype(_elem(sfx))
    Q[::4] = X[rng.choice(n, len(Q[::4]))]
    labels = repeated_labels(n, 31, 150)
    W = _shared_windows(labels, nq, 3)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    oi = getattr(oracle, "PrefilterIndex" + sfx)(X, labels)
    ctx = gu.RowContext(X.astype(np.float32), labels, Q.astype(np.float32), W, gu.metric_of(sfx), "prefilter")
    for k in (10, 1, 16):
        ids, dists, c = _both_paths(pi, wa, monkeypatch, Q, W, k)
        print(f"[typed dense] ties {sfx} d={d} k={k}: unproven {c['gemm_unproven']}, rescued {c['gemm_rescued']} of {c['gemm_queries']}")
        assert c["gemm_queries"] > nq // 2, c
        eids, edists = oi.batch_search(Q, W, nq, _qp(oracle, k))
        ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
        assert ok, f"{sfx} d={d} k={k}: {why}"


@pytest.mark.parametrize("sfx", ("UInt8Euclidian", "UInt8Mips", "Int8Euclidian", "Int8Mips"))
def test_typed_dense_prefilter_packs_queries_like_the_scan(wa, gpu, monkeypatch, sfx):
    """Device-buffer calls take fp32 queries as they are: fractional, negative and > 255 values become bytes by the exact scan's
    rule ((int)q & 0xff) inside the score kernel too."""
    import torch
    rng = np.random.default_rng(77)
    n, d, nq, k = 20000, 40, 200, 10
    X = _random_rows(sfx, rng, n, d)
    labels = rng.permutation(n).astype(np.float32)
    Q = (rng.random((nq, d)) * 700 - 250).astype(np.float32)  # [-250, 450): fractions, negatives, beyond both byte ranges
    Q[::5] = np.rint(Q[::5])
    W = np.zeros((nq, 2), dtype=np.float32)
    W[:120] = (1000.5, 9000.5)
    W[120:] = (12000.5, 14000.5)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    dev = torch.device("cuda:0")
    tq, tw = torch.from_numpy(Q).to(dev), torch.from_numpy(W).to(dev)
    rows = []
    for gemm in (True, False):
        if gemm:
            monkeypatch.delenv("WANN_NO_GEMM", raising=False)
        else:
            monkeypatch.setenv("WANN_NO_GEMM", "1")
        ti = torch.zeros((nq, k), dtype=torch.int32, device=dev)
        td = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        pi.batch_search_device(tq.data_ptr(), tw.data_ptr(), nq, 0, "", _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0)
        assert pi.counters()["gemm_queries"] == (nq if gemm else 0), pi.counters()
        rows.append((ti.cpu().numpy(), td.cpu().numpy()))
    assert np.array_equal(rows[0][1].view(np.uint32), rows[1][1].view(np.uint32))
    assert np.array_equal(rows[0][0], rows[1][0])


@pytest.mark.parametrize("sfx", ("UInt8Euclidian", "Int8Mips", "Float16Euclidian"))
def test_typed_batches_without_shared_windows_keep_their_counters(oracle, wa, gpu, monkeypatch, sfx):
    """No two windows alike: the dense path, tried on the batch, takes nothing and the exact scan does the oracle's work."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    rng = np.random.default_rng(9)
    n, d, nq = 30000, 32, 300
    X, Q = _random_rows(sfx, rng, n, d), _random_rows(sfx, rng, nq, d)
    labels = rng.permutation(n).astype(np.float32)
    W = np.stack([np.arange(nq) * 10.0 + 0.5, np.arange(nq) * 10.0 + 2000.5], 1)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    oi, oq = _oracle_index(oracle, sfx, X, labels)
    ids, dists = pi.batch_search(Q, W, nq, _qp(wa))
    c = pi.counters()
    eids, edists = oi.batch_search(Q.astype(oq), W, nq, _qp(oracle))
    ok, why = gu.same_rows(eids, edists, ids, dists, True,
                           gu.RowContext(X.astype(np.float32), labels, Q.astype(np.float32), W, gu.metric_of(sfx), "prefilter"))
    assert ok, why
    assert c["gemm_queries"] == 0 and c["dist_cmps"] + c["brute_rows"] == oi.last_counters["dist_cmps"], (c, oi.last_counters)


def test_typed_dense_prefilter_backs_off_on_streams_without_shared_windows(wa, gpu, monkeypatch):
    """The float32 test's stream on a uint8 index: after batches without any window group the dense path is tried every eighth
    batch only, picks up again when shared windows return, and the rows never depend on which path ran."""
    rng = np.random.default_rng(23)
    n, d, nq = 30000, 32, 400
    X, Q = _random_rows("UInt8", rng, n, d), _random_rows("UInt8", rng, nq, d)
    labels = rng.permutation(n).astype(np.float32)
    pi = wa.PrefilterIndexUInt8Euclidian(X, labels)
    distinct = np.stack([np.arange(nq) * 10.0 + 0.5, np.arange(nq) * 10.0 + 3000.5], 1)
    shared = np.tile(np.array([[100.5, 9100.5]]), (nq, 1))
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    want_d = pi.batch_search(Q, distinct, nq, _qp(wa))
    want_s = pi.batch_search(Q, shared, nq, _qp(wa))
    monkeypatch.delenv("WANN_NO_GEMM")
    got = pi.batch_search(Q, shared, nq, _qp(wa))
    assert pi.counters()["gemm_queries"] == nq
    assert np.array_equal(got[0], want_s[0]) and np.array_equal(got[1], want_s[1])
    for _ in range(3):
        got = pi.batch_search(Q, distinct, nq, _qp(wa))
        assert pi.counters()["gemm_queries"] == 0
        assert np.array_equal(got[0], want_d[0]) and np.array_equal(got[1], want_d[1])
    dense = []
    for _ in range(10):
        got = pi.batch_search(Q, shared, nq, _qp(wa))
        dense.append(pi.counters()["gemm_queries"])
        assert np.array_equal(got[0], want_s[0]) and np.array_equal(got[1], want_s[1])
    assert dense[0] == 0 and max(dense) == nq, dense          # skipped at first, picked up within eight batches ...
    assert dense[dense.index(nq):] == [nq] * (10 - dense.index(nq)), dense  # ... and then on every batch
