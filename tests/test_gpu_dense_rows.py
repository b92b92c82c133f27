"""GPU: the dense path's score launches read the one-byte copy of a float32 index's rows (include/wann.h, wann_set_dense_rows).

An integer 0 .. 255 is one bfloat16 value, so the score kernel of the copy (csrc/wann_gemm_kernels_w8.inc) is the bfloat16
kernel behind a fetch that widens bytes, and its accumulators hold the float32 kernel's values.  Norms, selection, proof and
re-rank keep the float32 rows.  So every batch is run on ONE index with the switch off and on, and ids, distance BITS and the
dense counters must be equal: no tolerance, no tie allowance (both paths order by (distance, id)).

Point sets are seeded random integers 0 .. 255 as float32 (0, 255 and values >= 128 included); queries are finite and NOT
integers -- data-like values plus noise, some rows negated, some scaled to a magnitude of 10^3.  Labels are a permutation of
0 .. n - 1 and a window is given by its positions [a, b) of the label order (util.pos_windows)."""
import ctypes

import numpy as np
import pytest

import golden_util as gu
from util import mixed_positions, pos_windows

pytestmark = pytest.mark.gpu

DENSE = ("gemm_queries", "gemm_unproven", "gemm_rescued")


def _qp(mod, k=10, beam=10):
    return mod.QueryParams(k, beam, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def _points(rng, n, d):
    X = rng.integers(0, 256, (n, d)).astype(np.float32)
    X[0, 0], X[1, 0], X[2, 0] = 0, 255, 128
    assert X.min() == 0 and X.max() == 255 and not np.signbit(X).any()
    return X


def _queries(rng, nq, d):
    Q = rng.integers(0, 256, (nq, d)).astype(np.float32) + (rng.random((nq, d), dtype=np.float32) - np.float32(0.5))
    Q[3::7] *= np.float32(-1)      # negative
    Q[5::11] *= np.float32(4.125)  # of magnitude 10^3
    assert np.isfinite(Q).all() and not np.array_equal(Q, np.rint(Q)) and np.abs(Q).max() > 900 and Q.min() < -200
    return Q


def _bits(r):
    return np.ascontiguousarray(r[0]).view(np.uint32), np.ascontiguousarray(r[1]).view(np.uint32)


def _same(r0, r1, what):
    (i0, d0), (i1, d1) = _bits(r0), _bits(r1)
    bad = np.nonzero((i0 != i1).any(axis=1) | (d0 != d1).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], r0[0][bad[:2]], r1[0][bad[:2]], r0[1][bad[:2]], r1[1][bad[:2]])


def _off_then_on(idx, search, what):
    """one batch with the switch off, then on: equal rows, equal dense counters, dense_rows 0 / 1; returns (rows, counters off)"""
    assert idx.set_dense_rows(False) is False
    r0 = search()
    c0 = idx.counters()
    assert c0["dense_rows"] == 0, what
    assert idx.set_dense_rows(True) is True and idx.dense_rows() is True, what
    try:
        r1 = search()
        c1 = idx.counters()
    finally:
        assert idx.set_dense_rows(False) is False
    print(f"[dense rows] {what}: off {[c0[f] for f in DENSE]} on {[c1[f] for f in DENSE]} dense_rows {c1['dense_rows']}")
    _same(r0, r1, what)
    for f in DENSE:
        assert c0[f] == c1[f], (what, f, c0[f], c1[f])
    return r0, c0, c1


# ---- 1. shared windows ------------------------------------------------------------------------------------------------------
N1 = 12000
# (width, start): the minimum width, widths around the 2 048-position chunk, and a window that ends at the last position
WINDOWS1 = [(1024, 100), (1500, 3001), (2048, 4096), (2049, 6144), (2600, 777), (5000, 6500), (1024, 2048), (2047, 5000), (3000, 8000),
            (4097, 1), (1300, 10000), (1500, N1 - 1500)]


def _shared_batch(rng, d):
    per = 25
    a = np.repeat([s for _, s in WINDOWS1], per)
    b = a + np.repeat([w for w, _ in WINDOWS1], per)
    assert b.max() == N1 and len(a) == 300
    perm = rng.permutation(len(a))
    return _queries(rng, len(a), d), pos_windows(a[perm], b[perm])


@pytest.mark.parametrize("d", (16, 40, 48, 100, 112, 128))
@pytest.mark.parametrize("sfx", ("FloatEuclidian", "FloatMips"))
def test_shared_windows(oracle, wa, gpu, monkeypatch, sfx, d):
    """d = 16: half a group of the copy; 48, 112: odd multiples of 16; 40, 100: the copy's padding; 128: four whole groups.
    The cap on gemm_unproven is asserted on the switch-off run -- the float32 kernels, which are not under test."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    rng = np.random.default_rng(1000 + d)
    X = _points(rng, N1, d)
    labels = rng.permutation(N1).astype(np.float32)
    Q, W = _shared_batch(rng, d)
    nq = len(Q)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    assert pi.dense_rows() is False and pi.dense_rows_bytes() == N1 * 64 * ((d + 63) // 64)
    for k in (1, 10, 16):
        r0, c0, c1 = _off_then_on(pi, lambda: pi.batch_search(Q, W, nq, _qp(wa, k)), f"shared {sfx} d={d} k={k}")
        assert c0["gemm_queries"] == nq, c0
        assert c0["gemm_unproven"] <= c0["gemm_queries"] // 10, c0
        assert c1["dense_rows"] == 1
        if d == 100 and k == 10:
            oi = getattr(oracle, "PrefilterIndex" + sfx)(X, labels)
            eids, edists = oi.batch_search(Q, W, nq, _qp(oracle, k))
            ctx = gu.RowContext(X, labels, Q, W, gu.metric_of(sfx), "prefilter")
            ok, why = gu.same_rows(eids, edists, r0[0], r0[1], True, ctx)
            assert ok, f"{sfx} d={d} k={k}: {why}"


# ---- 2. position probe ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (48, 128))
@pytest.mark.parametrize("sfx", ("FloatEuclidian", "FloatMips"))
def test_position_probe(wa, gpu, monkeypatch, sfx, d):
    """Every row is the base row (100 everywhere) but for a few elements.  For every element e, 12 rows carry 250 at e and a small
    difference 1 + j at element e + 7; the other rows carry small negative differences in elements 0 .. 2 (all rows distinct).
    A query is the base with a large value at ONE element e (16 queries per element, one shared window over the whole set): its
    neighbours are the 12 rows of e.  A kernel that stages any element of a row at another position scores those rows like all
    the others there and selects other candidates."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    rng = np.random.default_rng(50 + d)
    per, qper, k = 12, 16, 10
    n = d * per + 1500 + 37
    X = np.full((n, d), 100, dtype=np.float32)
    for e in range(d):
        for j in range(per):
            X[e * per + j, e] = 250
            X[e * per + j, (e + 7) % d] += 1 + j
    i = np.arange(n - d * per)
    X[d * per:, 0] -= 1 + i % 20
    X[d * per:, 1] -= 1 + (i // 20) % 20
    X[d * per:, 2] -= 1 + i // 400
    assert len(np.unique(X, axis=0)) == n and X.min() >= 0 and X.max() <= 255
    order = rng.permutation(n)
    X = X[order]
    labels = rng.permutation(n).astype(np.float32)
    nq = d * qper
    Q = np.full((nq, d), 100.25, dtype=np.float32) + (rng.random((nq, d), dtype=np.float32) - np.float32(0.5)) * np.float32(0.25)
    probe = np.repeat(np.arange(d), qper)
    Q[np.arange(nq), probe] = np.float32(250.5)
    W = pos_windows(np.zeros(nq, dtype=np.int64), np.full(nq, n - 1))
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    r0, c0, c1 = _off_then_on(pi, lambda: pi.batch_search(Q, W, nq, _qp(wa, k)), f"probe {sfx} d={d}")
    assert c0["gemm_queries"] == nq and c1["dense_rows"] == 1
    assert c0["gemm_unproven"] <= nq // 10, c0
    # the rows are the probed element's
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)  # inv[original row] = row of X
    for q in range(0, nq, 5):
        want = set(inv[probe[q] * per:probe[q] * per + per].tolist())
        assert set(r0[0][q].tolist()) <= want, (q, probe[q], r0[0][q])
    # ... and the exact scan's
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    scan = pi.batch_search(Q, W, nq, _qp(wa, k))
    assert pi.counters()["gemm_queries"] == 0
    _same(r0, scan, f"probe {sfx} d={d} against the scan")


# ---- 3. cover groups --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (40, 128))
def test_cover_groups(wa, gpu, monkeypatch, d):
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work)
    rng = np.random.default_rng(300 + d)
    n, nq, k = 30000 + 777, 1200, 10
    X = _points(rng, n, d)
    labels = rng.permutation(n).astype(np.float32)
    Q = _queries(rng, nq, d)
    a, b = mixed_positions(rng, n, nq)
    W = pos_windows(a, b)
    pi = wa.PrefilterIndexFloatEuclidian(X, labels)
    pi.set_dense_windows(True)
    covers = []

    def search():
        r = pi.batch_search(Q, W, nq, _qp(wa, k))
        covers.append(pi.dense_window_counters())
        return r

    r0, c0, c1 = _off_then_on(pi, search, f"cover d={d}")
    print(f"[dense rows] cover d={d}: {covers}")
    assert covers[0]["queries"] > nq // 2, covers
    for f in covers[0]:
        assert covers[0][f] == covers[1][f], (f, covers)
    assert c1["dense_rows"] == 1 and c0["brute_rows"] == c1["brute_rows"]


# ---- 4. exact windows on the tree kinds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,d", (("VamanaRangeFilterTreeIndex", 100), ("SuperOptimizedPostfilterTreeIndex", 48)))
def test_exact_windows_on_the_tree_kinds(wa, gpu, monkeypatch, tmp_path, family, d):
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.delenv("WANN_DENSE_ALWAYS", raising=False)
    rng = np.random.default_rng(400 + d)
    n, k, L = 12000, 10, 4096
    X = _points(rng, n, d)
    labels = rng.permutation(n).astype(np.float32)
    # four shared windows of 20 queries, and 160 windows of their own: 1 100 .. 3 500 positions, all below L
    sa = np.array([200, 3000, 6000, 8500])
    sw = np.array([1024, 2049, 1500, 3300])
    w = np.concatenate([np.repeat(sw, 20), rng.integers(1100, 3501, 160)])
    a = np.concatenate([np.repeat(sa, 20), (rng.random(160) * (n - 3600)).astype(np.int64) + 1])
    perm = rng.permutation(len(a))
    a, w = a[perm], w[perm]
    nq = len(a)
    assert nq >= 64 and w.max() < L
    Q, W = _queries(rng, nq, d), pos_windows(a, a + w)
    bp = wa.BuildParams(32, 64, 1.0, "")
    tree = family.startswith("Vamana")
    if tree:
        idx = getattr(wa, family + "FloatEuclidian")(X, labels, cutoff=1000, split_factor=2, build_params=bp)
    else:
        idx = getattr(wa, family + "FloatEuclidian")(X, labels, cutoff=1000, split_factor=2, shift_factor=0.5, build_params=bp)
    assert idx.byte_rows_bytes() == n * 64 * ((d + 63) // 64) and idx.dense_rows_bytes() == idx.byte_rows_bytes()
    assert idx.dense_rows() is False and idx.set_exact_windows(L) == 0
    args = ("optimized_postfilter",) if tree else ()
    runs = {}
    try:
        for byte_rows in (False, True):
            for dense_rows in (False, True):
                assert idx.set_byte_rows(byte_rows) is byte_rows and idx.set_dense_rows(dense_rows) is dense_rows
                r = idx.batch_search(Q, W, nq, *args, _qp(wa, k))
                runs[(byte_rows, dense_rows)] = (r, idx.exact_window_counters(), idx.counters())
    finally:
        idx.set_byte_rows(False)
        idx.set_dense_rows(False)
        idx.set_exact_windows(0)
    r00, e00, c00 = runs[(False, False)]
    print(f"[dense rows] exact windows {family} d={d}: {e00}")
    assert e00["queries"] == nq and e00["dense_queries"] > 0, e00
    for key, (r, e, c) in runs.items():
        _same(r00, r, (family, key))
        assert e == e00, (key, e, e00)
        assert c["dense_rows"] == (1 if key[1] else 0), (key, c)
        for f in DENSE:
            assert c[f] == c00[f], (key, f)


# ---- 5. refusals and bookkeeping --------------------------------------------------------------------------------------------
def _small_batch(rng, n, d, nq_per=20):
    a = np.repeat([10, 1200], nq_per)
    b = a + np.repeat([1100, 1500], nq_per)
    assert b.max() < n
    return _queries(rng, len(a), d), pos_windows(a, b)


def _refused(idx, search, what):
    """no copy: the switch stays off, and a batch is what it was"""
    assert idx.dense_rows_bytes() == 0, what
    r0 = search()
    c0 = idx.counters()
    assert idx.set_dense_rows(True) is False and idx.dense_rows() is False, what
    r1 = search()
    c1 = idx.counters()
    _same(r0, r1, what)
    assert c0["dense_rows"] == 0 and c1["dense_rows"] == 0, what
    for f in DENSE:
        assert c0[f] == c1[f], (what, f)
    return c0


def test_points_that_are_not_byte_exact_are_refused(wa, gpu, monkeypatch):
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    n, d = 3000, 32
    minus_zero = np.array([0x80000000], dtype=np.uint32).view(np.float32)[0]
    for name, bad in (("0.5", np.float32(0.5)), ("256", np.float32(256)), ("-1", np.float32(-1)), ("-0.0", minus_zero)):
        rng = np.random.default_rng(7)
        X = _points(rng, n, d)
        X[n - 1, d - 1] = bad
        assert name != "-0.0" or (X[n - 1, d - 1] == 0 and np.signbit(X[n - 1, d - 1]))
        labels = rng.permutation(n).astype(np.float32)
        Q, W = _small_batch(rng, n, d)
        pi = wa.PrefilterIndexFloatEuclidian(X, labels)
        c = _refused(pi, lambda: pi.batch_search(Q, W, len(Q), _qp(wa)), "bad value " + name)
        assert c["gemm_queries"] == len(Q), (name, c)  # (the float32 dense path took the batch)


def test_kinds_types_and_row_lengths_without_a_copy(wa, gpu, monkeypatch):
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    rng = np.random.default_rng(8)
    n = 3000
    labels = rng.permutation(n).astype(np.float32)
    bp = wa.BuildParams(32, 64, 1.0, "")
    # rows of 200 elements: a PrefilterIndex, and a tree index -- which HAS one-byte shadow rows, but none this path can read
    X200 = _points(rng, n, 200)
    Q200, W200 = _small_batch(rng, n, 200)
    pi = wa.PrefilterIndexFloatEuclidian(X200, labels)
    c = _refused(pi, lambda: pi.batch_search(Q200, W200, len(Q200), _qp(wa)), "PrefilterIndex d=200")
    assert c["gemm_queries"] == len(Q200)
    tree = wa.VamanaRangeFilterTreeIndexFloatEuclidian(X200, labels, cutoff=1000, split_factor=2, build_params=bp)
    assert tree.byte_rows_bytes() > 0
    assert tree.set_exact_windows(2048) == 0
    _refused(tree, lambda: tree.batch_search(Q200, W200, len(Q200), "optimized_postfilter", _qp(wa)), "tree d=200")
    assert tree.exact_window_counters()["dense_queries"] == len(Q200)
    # kinds without a dense path, element types without a copy
    X = _points(rng, n, 32)
    Q, W = _small_batch(rng, n, 32)
    post = wa.PostfilterVamanaIndexFloatEuclidian(X, labels, bp)
    assert post.byte_rows_bytes() > 0
    _refused(post, lambda: post.batch_search(Q, W, len(Q), _qp(wa)), "PostfilterVamanaIndex")
    leaf = wa.RangeFilterTreeIndexFloatMips(X, labels, cutoff=1000, split_factor=2)
    _refused(leaf, lambda: leaf.batch_search(Q, W, len(Q), "optimized_postfilter", _qp(wa)), "RangeFilterTreeIndex")
    for sfx, elem in (("UInt8Euclidian", np.uint8), ("Float16Euclidian", np.float16)):
        pi = getattr(wa, "PrefilterIndex" + sfx)(X.astype(elem), labels)
        Qe = np.abs(np.rint(Q)).clip(0, 255).astype(elem)
        _refused(pi, lambda: pi.batch_search(Qe, W, len(Qe), _qp(wa)), "PrefilterIndex" + sfx)
    assert np.array_equal(wa.bfloat16_round(X), X)  # (integers 0 .. 255 are bfloat16 values)
    bf = wa.PrefilterIndexBFloat16Euclidian(X, labels)
    Qb = wa.bfloat16_round(Q)
    _refused(bf, lambda: bf.batch_search(Qb, W, len(Qb), _qp(wa)), "PrefilterIndexBFloat16")


def test_bookkeeping_of_an_eligible_prefilter_index(wa, gpu, monkeypatch):
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    rng = np.random.default_rng(9)
    n, d = 3000, 100
    X = _points(rng, n, d)
    labels = rng.permutation(n).astype(np.float32)
    pi = wa.PrefilterIndexFloatMips(X, labels)
    assert pi.dense_rows_bytes() == n * 64 * ((d + 63) // 64)
    assert pi.byte_rows_bytes() == 0 and pi.set_byte_rows(True) is False and pi.set_scan_rows(True) is False
    before = pi.device_bytes()
    assert pi.set_dense_rows(True) is True and pi.device_bytes() == before
    # 64 windows of their own: the dense launches find no group, no score launch reads a row
    a = 5 + 17 * np.arange(64)
    Q, W = _queries(rng, 64, d), pos_windows(a, a + 1100 + np.arange(64))
    pi.batch_search(Q, W, 64, _qp(wa))
    c = pi.counters()
    assert c["gemm_queries"] == 0 and c["dense_rows"] == 0 and c["brute_rows"] > 0, c
    Q, W = _small_batch(rng, n, d)
    pi.batch_search(Q, W, len(Q), _qp(wa))
    assert pi.counters()["dense_rows"] == 1
    assert pi.set_dense_rows(False) is False and pi.device_bytes() == before
    pi.batch_search(Q, W, len(Q), _qp(wa))
    assert pi.counters()["dense_rows"] == 0


class _QP(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int64), ("beam_width", ctypes.c_int64), ("cut", ctypes.c_double), ("limit", ctypes.c_int64),
                ("degree_limit", ctypes.c_int64), ("final_beam_multiply", ctypes.c_int64), ("postfiltering_max_beam", ctypes.c_int64),
                ("has_ratio", ctypes.c_int32), ("ratio", ctypes.c_float), ("verbose", ctypes.c_int32)]


def test_every_call_form(wa, gpu, monkeypatch):
    """one eligible batch through the host call, the device call, the asynchronous device call + wait, and the C ABI"""
    torch = pytest.importorskip("torch")
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    rng = np.random.default_rng(10)
    n, d, k = 3000, 48, 10
    X = np.ascontiguousarray(_points(rng, n, d))
    labels = rng.permutation(n).astype(np.float32)
    Q, W = _small_batch(rng, n, d)
    Q, Wf = np.ascontiguousarray(Q), np.ascontiguousarray(W.astype(np.float32))
    nq = len(Q)
    pi = wa.PrefilterIndexFloatEuclidian(X, labels)
    want = pi.batch_search(Q, W, nq, _qp(wa, k))
    assert pi.counters()["dense_rows"] == 0 and pi.counters()["gemm_queries"] == nq
    assert pi.set_dense_rows(True) is True
    _same(want, pi.batch_search(Q, W, nq, _qp(wa, k)), "host call")
    assert pi.counters()["dense_rows"] == 1
    dev = torch.device("cuda:0")
    tq, tw = torch.from_numpy(Q).to(dev), torch.from_numpy(Wf).to(dev)

    def outputs():
        return torch.zeros((nq, k), dtype=torch.int32, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev)

    ti, td = outputs()
    torch.cuda.synchronize()
    pi.batch_search_device(tq.data_ptr(), tw.data_ptr(), nq, 0, "", _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0)
    _same(want, (ti.cpu().numpy().view(np.uint32), td.cpu().numpy()), "device call")
    assert pi.counters()["dense_rows"] == 1
    # submitted with the switch on, waited for with it off: the batch keeps what it was submitted with
    ti, td = outputs()
    torch.cuda.synchronize()
    ticket = pi.batch_search_device_async(tq.data_ptr(), tw.data_ptr(), nq, 0, "", _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0)
    assert pi.set_dense_rows(False) is False
    c = pi.wait(ticket)
    _same(want, (ti.cpu().numpy().view(np.uint32), td.cpu().numpy()), "asynchronous call")
    assert c["dense_rows"] == 1 and c["gemm_queries"] == nq
    # the C ABI
    import rangefilteredann_amd
    lib = ctypes.CDLL(rangefilteredann_amd.lib_path())
    lib.wann_index_create.restype = ctypes.c_void_p
    lib.wann_index_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.wann_index_destroy.argtypes = [ctypes.c_void_p]
    lib.wann_set_dense_rows.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for f in (lib.wann_dense_rows, lib.wann_last_dense_rows, lib.wann_dense_rows_bytes, lib.wann_byte_rows_bytes):
        f.argtypes = [ctypes.c_void_p]
    lib.wann_dense_rows_bytes.restype = ctypes.c_int64
    lib.wann_byte_rows_bytes.restype = ctypes.c_int64
    lib.wann_batch_search.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_char_p] + [ctypes.c_void_p] * 3
    h = lib.wann_index_create(0, 0, 0, X.ctypes.data, n, d, labels.ctypes.data, 1000, 2.0, 0.5, None, 0, 4)
    assert h
    try:
        assert lib.wann_dense_rows(h) == 0 and lib.wann_dense_rows_bytes(h) == n * 64 and lib.wann_byte_rows_bytes(h) == 0
        qp = _QP(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, 0, 0.0, 0)
        for on in (0, 1):
            assert lib.wann_set_dense_rows(h, on) == on and lib.wann_dense_rows(h) == on
            ids = np.zeros((nq, k), dtype=np.uint32)
            dists = np.zeros((nq, k), dtype=np.float32)
            assert lib.wann_batch_search(h, Q.ctypes.data, Wf.ctypes.data, nq, b"", ctypes.byref(qp), ids.ctypes.data, dists.ctypes.data) == 0
            assert lib.wann_last_dense_rows(h) == on
            _same(want, (ids, dists), f"C ABI, switch {on}")
    finally:
        lib.wann_index_destroy(h)
