"""GPU: the dense (MFMA) prefilter path on float8 point sets (OCP E4M3; rows of at most 128 elements).

An E4M3 value has four significant bits, so it is exactly one bfloat16 value: a float8 row is its own high bf16 term.  The score
kernel is the bfloat16 one behind the byte fetch of the one-byte rows -- one staged row per point, two products per step -- and
its accumulators hold the float32 kernel's values on the upcast row; norms, selection, re-rank and rescue read the float8 rows.
So a batch returns exactly the rows (ids and distance bits) of the exact scan (WANN_NO_GEMM=1) and of the float32 index on the
upcast points, with that index's dense counters."""
import numpy as np
import pytest

import golden_util as gu
from util import clustered_window_batch, pos_windows, random_rows, repeated_labels

pytestmark = pytest.mark.gpu

CLASSES = ("Float8Euclidian", "Float8Mips")
SCALE = np.float32(8.0)  # unit rows times a power of two: components of about 8 / sqrt(d) sit in E4M3's normal range; no ordering changes


def _qp(mod, k=10):
    return mod.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def _f32(sfx):
    return sfx.replace("Float8", "Float")


def _unit8(wa, rng, n, d):
    """well-spread rows: unit vectors scaled by SCALE, rounded to float8 (float32 arrays)"""
    return wa.float8_round(random_rows("Float", rng, n, d) * SCALE)


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


def _families(nq=700):
    W = np.zeros((nq, 2))
    W[:300] = (100.5, 25100.5)       # 25 000 positions: eight slices of 3 200; three query tiles
    W[300:520] = (30000.5, 35000.5)  # 5 000 positions: three slices; two tiles
    W[520:560] = (-1, 1e9)           # everything
    W[560:660] = (500.5, 1800.5)     # 1 300 positions: one short slice
    W[660:] = (7.5, 250.5)           # below the minimum window: exact scan
    return W


@pytest.mark.parametrize("d", (16, 40, 100, 128))
@pytest.mark.parametrize("sfx", CLASSES)
def test_float8_dense_prefilter_slices_and_tiles(wa, gpu, monkeypatch, sfx, d):
    """The window families of test_bfloat16_dense_prefilter_slices_and_tiles and a block of duplicated rows, at d = 16 (one
    k-step, half a 32-element group), 40 (not a multiple of 16), 100 (the <112> kernel) and 128 (four whole groups).  A condition
    on the INPUT first: the float32 index on the same upcast rows sends fewer than a tenth of the 660 dense queries back to the
    scan.  Then the float8 index: the exact scan's rows, the float32 index's rows, the float32 index's counters."""
    rng = np.random.default_rng(5)
    n, nq = 42000, 700
    X, Q = _unit8(wa, rng, n, d), _unit8(wa, rng, nq, d)
    X[1000:1040] = X[1000]  # duplicates
    labels = rng.permutation(n).astype(np.float32)
    W = _families(nq)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    f32 = getattr(wa, "PrefilterIndex" + _f32(sfx))(X, labels)
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    for k in (10, 1):
        fids, fdists = f32.batch_search(Q, W, nq, _qp(wa, k))
        fc = f32.counters()
        assert fc["gemm_queries"] == 660 and fc["gemm_unproven"] < 66, fc  # (the input's condition, on existing code)
        ids, dists, c = _both_paths(pi, wa, monkeypatch, Q, W, k)
        print(f"[float8 dense] {sfx} d={d} k={k}: unproven {c['gemm_unproven']}, rescued {c['gemm_rescued']} of {c['gemm_queries']}; "
              f"float32: unproven {fc['gemm_unproven']}, rescued {fc['gemm_rescued']} of {fc['gemm_queries']}")
        assert np.array_equal(fids, ids) and np.array_equal(fdists.view(np.uint32), dists.view(np.uint32)), k
        assert (c["gemm_queries"], c["gemm_unproven"], c["gemm_rescued"]) == (fc["gemm_queries"], fc["gemm_unproven"], fc["gemm_rescued"]), (fc, c)


def dense_batch(wa, sfx):
    """util.clustered_window_batch rounded to float8: SIFT-like integers halved (0 .. 127.5: E4M3 keeps four significant bits) for
    squared L2, unit rows times SCALE for the inner product"""
    if sfx.endswith("Euclidian"):
        X, Q, labels, W = clustered_window_batch(128, "sift")
        X, Q = X * np.float32(0.5), Q * np.float32(0.5)
    else:
        X, Q, labels, W = clustered_window_batch(100, "unit")
        X, Q = X / np.linalg.norm(X, axis=1, keepdims=True) * SCALE, Q / np.linalg.norm(Q, axis=1, keepdims=True) * SCALE
    return wa.float8_round(X), wa.float8_round(Q), labels, W


@pytest.mark.parametrize("sfx", CLASSES)
def test_float8_dense_prefilter_matches_oracle(oracle, wa, gpu, monkeypatch, sfx):
    """Clustered labels = clustered geometry, 40 queries per cluster window: rows are the exact scan's, the oracle's up to its
    ties, and the float32 index's on the upcast points -- as are the dense counters"""
    X, Q, labels, W = dense_batch(wa, sfx)
    nq = Q.shape[0]
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    f32 = getattr(wa, "PrefilterIndex" + _f32(sfx))(X, labels)
    oi = getattr(oracle, "PrefilterIndex" + _f32(sfx))(X, labels)
    ctx = gu.RowContext(X, labels, Q, W, gu.metric_of(sfx), "prefilter")
    for k in (1, 10, 16):
        ids, dists, c = _both_paths(pi, wa, monkeypatch, Q, W, k)
        print(f"[float8 dense] {sfx} k={k}: {c['gemm_queries']} of {nq} dense, unproven {c['gemm_unproven']}, rescued {c['gemm_rescued']}")
        assert c["gemm_queries"] > nq // 2, c
        eids, edists = oi.batch_search(Q, W, nq, _qp(oracle, k))
        ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
        assert ok, f"{sfx} k={k}: {why}"
        fids, fdists = f32.batch_search(Q, W, nq, _qp(wa, k))
        fc = f32.counters()
        assert (fc["gemm_queries"], fc["gemm_unproven"], fc["gemm_rescued"]) == (c["gemm_queries"], c["gemm_unproven"], c["gemm_rescued"]), (fc, c)
        assert np.array_equal(fdists.view(np.uint32), dists.view(np.uint32)), k


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
@pytest.mark.parametrize("sfx", CLASSES)
def test_float8_dense_prefilter_ties(oracle, wa, gpu, monkeypatch, sfx, d):
    """Three-valued elements (-1, 0, 1: float8-exact) and repeated labels: most queries have many points at their k-th distance.
    Rows equal the exact scan's bit for bit and the oracle's up to its ties."""
    rng = np.random.default_rng(41 + d)
    n, nq = 20000, 400
    X = rng.integers(-1, 2, (n, d)).astype(np.float32)
    Q = rng.integers(-1, 2, (nq, d)).astype(np.float32)
    Q[::4] = X[rng.choice(n, len(Q[::4]))]
    assert np.array_equal(wa.float8_round(X), X)
    labels = repeated_labels(n, 31, 150)
    W = _shared_windows(labels, nq, 3)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    oi = getattr(oracle, "PrefilterIndex" + _f32(sfx))(X, labels)
    ctx = gu.RowContext(X, labels, Q, W, gu.metric_of(sfx), "prefilter")
    for k in (10, 1, 16):
        ids, dists, c = _both_paths(pi, wa, monkeypatch, Q, W, k)
        print(f"[float8 dense] ties {sfx} d={d} k={k}: unproven {c['gemm_unproven']}, rescued {c['gemm_rescued']} of {c['gemm_queries']}")
        assert c["gemm_queries"] > nq // 2, c
        eids, edists = oi.batch_search(Q, W, nq, _qp(oracle, k))
        ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
        assert ok, f"{sfx} d={d} k={k}: {why}"


def _distinct_windows(labels, nq, seed, lo=1100, hi=9000):
    """windows of lo .. hi points with ends from the sorted labels, no two made alike on purpose"""
    rng = np.random.default_rng(seed)
    s = np.sort(labels)
    n = len(s)
    W = np.zeros((nq, 2))
    for i in range(nq):
        w = int(rng.integers(lo, hi))
        st = int(rng.integers(0, n - w))
        W[i] = (s[st], s[st + w])
    return W


@pytest.mark.parametrize("sfx,d", [("Float8Euclidian", 100), ("Float8Mips", 48)])
def test_float8_distinct_wide_windows(wa, gpu, monkeypatch, sfx, d):
    """set_dense_windows(True) on a float8 PrefilterIndex (20 000 points, 600 distinct windows; WANN_DENSE_ALWAYS lifts the
    minimum on the batch's scan work): the cover path takes most of the batch and the rows are those of the option off"""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    rng = np.random.default_rng(101 + d)
    n, nq = 20000, 600
    X, Q = _unit8(wa, rng, n, d), _unit8(wa, rng, nq, d)
    labels = rng.permutation(n).astype(np.float32)
    W = _distinct_windows(labels, nq, 3)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    for k in (10, 1):
        pi.set_dense_windows(False)
        ids0, d0 = pi.batch_search(Q, W, nq, _qp(wa, k))
        c0 = pi.counters()
        assert pi.dense_window_counters()["queries"] == 0
        assert pi.set_dense_windows(True) is False
        ids1, d1 = pi.batch_search(Q, W, nq, _qp(wa, k))
        c1, w1 = pi.counters(), pi.dense_window_counters()
        print(f"[float8 dense] windows {sfx} d={d} k={k}: cover {w1}, brute_rows {c0['brute_rows']} -> {c1['brute_rows']}")
        assert np.array_equal(ids0, ids1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32)), (k, w1)
        assert w1["queries"] > nq // 2, w1
        assert c1["brute_rows"] < c0["brute_rows"]


def test_float8_exact_windows(wa, gpu, tmp_path, monkeypatch):
    """set_exact_windows(4096) on a float8 graph-backed tree (20 000 points, 600 windows of 300 .. 6 000 positions): dense and
    scan-only rows are equal, and equal to a float8 PrefilterIndex's"""
    n, nq, k, L, d = 20000, 600, 10, 4096, 100
    rng = np.random.default_rng(5)
    X = _unit8(wa, rng, n, d)
    labels = rng.permutation(n).astype(np.float32)
    rng = np.random.default_rng(55)
    Q = _unit8(wa, rng, nq, d)
    w = rng.integers(300, 6001, nq)
    a = (rng.random(nq) * (n - w - 2)).astype(np.int64) + 1
    W = pos_windows(a, a + w)
    small = w <= L
    idx = wa.VamanaRangeFilterTreeIndexFloat8Euclidian(X, labels, cutoff=1000, split_factor=2,
                                                      build_params=wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/"))
    search = lambda: idx.batch_search(Q, W, nq, "optimized_postfilter", _qp(wa, k))  # noqa: E731
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    off = search()
    assert idx.set_exact_windows(L) == 0
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    scan = search()
    es = idx.exact_window_counters()
    assert es["queries"] == int(small.sum()) and es["dense_queries"] == 0, es
    monkeypatch.delenv("WANN_NO_GEMM")
    dense = search()
    ed = idx.exact_window_counters()
    print(f"[float8 dense] exact windows: {ed}; scan-only rows_scanned {es['rows_scanned']}")
    assert ed["queries"] == int(small.sum()) and ed["dense_queries"] > 0, ed
    assert np.array_equal(scan[0], dense[0]) and np.array_equal(scan[1].view(np.uint32), dense[1].view(np.uint32))
    assert np.array_equal(off[0][~small], dense[0][~small]) and np.array_equal(off[1][~small].view(np.uint32), dense[1][~small].view(np.uint32))
    pi = wa.PrefilterIndexFloat8Euclidian(X, labels)
    pids, pd = pi.batch_search(Q, W, nq, _qp(wa, k))
    ctx = gu.RowContext(X, labels, Q[small], W[small], gu.metric_of("Euclidian"), "prefilter")
    ok, why = gu.same_rows(pids[small], pd[small], dense[0][small], dense[1][small], True, ctx)
    assert ok, why
    assert idx.set_exact_windows(0) == L


@pytest.mark.parametrize("long_rows", (False, True))
@pytest.mark.parametrize("sfx", CLASSES)
def test_float8_long_rows_keep_the_scan(oracle, wa, gpu, monkeypatch, sfx, long_rows):
    """rows of 256 elements are beyond the float8 dense kernel, with and without WANN_DENSE_LONG_ROWS: the shared-window batch
    takes the exact scan (gemm_queries == 0) and returns the oracle's rows"""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    if long_rows:
        monkeypatch.setenv("WANN_DENSE_LONG_ROWS", "1")
    else:
        monkeypatch.delenv("WANN_DENSE_LONG_ROWS", raising=False)
    rng = np.random.default_rng(8)
    n, nq, d = 12000, 200, 256
    X, Q = _unit8(wa, rng, n, d), _unit8(wa, rng, nq, d)
    labels = rng.permutation(n).astype(np.float32)
    W = np.zeros((nq, 2))
    W[:120] = (1000.5, 7000.5)
    W[120:] = (8000.5, 11000.5)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    oi = getattr(oracle, "PrefilterIndex" + _f32(sfx))(X, labels)
    ids, dists = pi.batch_search(Q, W, nq, _qp(wa))
    c = pi.counters()
    assert c["gemm_queries"] == 0, c
    eids, edists = oi.batch_search(Q, W, nq, _qp(oracle))
    ok, why = gu.same_rows(eids, edists, ids, dists, True, gu.RowContext(X, labels, Q, W, gu.metric_of(sfx), "prefilter"))
    assert ok, why
