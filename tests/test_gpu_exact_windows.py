"""GPU: the exact-window limit of the graph-backed tree indexes (`set_exact_windows`).

With a limit L > 0 a query whose window holds 0 < w <= L points is answered exactly -- the k nearest in-window points, ordered by
(distance, sorted position), ids through the decoding -- by the exact scan or, in a batch of 32 queries or more, by the dense
prefilter path on the matrix cores; both return the same rows bit for bit.  Every other query takes the ordinary path and returns
the ordinary rows bit for bit.

Labels are a permutation of 0 .. n - 1 and a window is given by its positions [a, b) of the label order, with ends between two
labels: the inclusive rule of util.brute_force_gt, the half-open rule of the tree's exact scan and (away from the last point)
PrefilterIndex's rule then name the same points."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
from util import REPO, brute_force_gt, pos_windows as _pos_windows, random_rows as _random_rows, recall, repeated_labels, tie_heavy, tie_queries
from util import wide_window_batch as _used_batch

pytestmark = pytest.mark.gpu

BLOCK = 2048  # kGemmPointChunk
ZERO = dict(queries=0, dense_queries=0, unproven=0, rescued=0, passes=0, rows_scanned=0)
WORK = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads", "gemm_queries", "gemm_unproven", "gemm_rescued")  # (the reference's operation counts)
FLT_MAX = np.finfo(np.float32).max


def _qp(mod, k=10, beam=10):
    return mod.QueryParams(k, beam, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def _elem(sfx):
    return np.uint8 if sfx.startswith("UInt8") else np.int8 if sfx.startswith("Int8") else np.float16 if sfx.startswith("Float16") else np.float32


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("exact_windows_graphs"))


_sets = {}


def _point_set(sfx, d, n, seed):
    """(X, labels) of one test input, generated once"""
    key = (sfx, d, n, seed)
    if key not in _sets:
        rng = np.random.default_rng(seed)
        _sets[key] = (_random_rows(sfx, rng, n, d), rng.permutation(n).astype(np.float32))
    return _sets[key]


def _index(wa, cache, family, sfx, X, labels, tag, cutoff=1000):
    path = os.path.join(cache, tag, "")
    os.makedirs(path, exist_ok=True)
    bp = wa.BuildParams(32, 64, 1.0, path)
    if family == "super":
        return getattr(wa, "SuperOptimizedPostfilterTreeIndex" + sfx)(X, labels, cutoff=cutoff, split_factor=2, shift_factor=0.5, build_params=bp)
    return getattr(wa, "VamanaRangeFilterTreeIndex" + sfx)(X, labels, cutoff=cutoff, split_factor=2, build_params=bp)


def _search(idx, family, Q, W, qp, method="optimized_postfilter"):
    if family == "super":
        return idx.batch_search(Q, W, len(Q), qp)
    return idx.batch_search(Q, W, len(Q), method, qp)


def _bits_equal(r0, r1, rows=slice(None)):
    return np.array_equal(r0[0][rows], r1[0][rows]) and np.array_equal(r0[1][rows].view(np.uint32), r1[1][rows].view(np.uint32))


def _record(line):
    print("[exact windows] " + line)
    out = os.environ.get("EXACT_WINDOWS_COUNTERS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


# ---- 1. exact rows ----------------------------------------------------------------------------------------------------------
ROW_CASES = [("tree", "FloatEuclidian", 64), ("tree", "FloatMips", 100), ("tree", "Float16Euclidian", 100), ("tree", "UInt8Euclidian", 100),
             ("tree", "Int8Mips", 100), ("super", "FloatMips", 100), ("super", "UInt8Euclidian", 100)]


@pytest.mark.parametrize("family,sfx,d", ROW_CASES)
def test_small_windows_return_the_exact_rows(wa, gpu, cache, monkeypatch, family, sfx, d):
    """600 queries, windows of 300 .. 6 000 positions, L = 4 096, beam 10.  The seeds (5 for the points, 55 for the batch): at
    beam 10 the post-filter search misses true neighbours of most of these windows -- the CPU oracle's
    VamanaRangeFilterTreeIndexFloatEuclidian on exactly these inputs (d = 64) has recall@10 0.768 on the 383 queries with w <= L and
    336 of their rows miss a neighbour -- so the option-off rows differ from the exact rows, which the test asserts.  No query of
    any case has its 10th and 11th nearest in-window points at one distance (checked in float64), so recall 1.0 is what an exact
    answer scores."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.delenv("WANN_DENSE_ALWAYS", raising=False)
    n, nq, k, L = 20000, 600, 10, 4096
    X, labels = _point_set(sfx, d, n, 5)
    rng = np.random.default_rng(55)
    Q = _random_rows(sfx, rng, nq, d)
    w = rng.integers(300, 6001, nq)
    a = (rng.random(nq) * (n - w - 2)).astype(np.int64) + 1  # (never the last point of the label order: PrefilterIndex drops it)
    W = _pos_windows(a, a + w)
    small = w <= L
    assert 100 < small.sum() < nq - 100
    idx = _index(wa, cache, family, sfx, X, labels, f"{family}-{sfx}-{d}")
    off = _search(idx, family, Q, W, _qp(wa, k))
    assert idx.exact_window_counters() == ZERO
    assert idx.set_exact_windows(L) == 0
    on = _search(idx, family, Q, W, _qp(wa, k))
    ec = idx.exact_window_counters()
    _record(f"rows {family} {sfx} d={d}: {ec}")
    assert ec["queries"] == int(small.sum()), ec
    # w > L: the option-off rows, bit for bit
    assert _bits_equal(off, on, ~small)
    # w <= L: a PrefilterIndex of the same data
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    pids, pd = pi.batch_search(Q, W, nq, _qp(wa, k))
    ctx = gu.RowContext(X.astype(np.float32), labels, Q.astype(np.float32)[small], W[small], gu.metric_of(sfx), "prefilter")
    ok, why = gu.same_rows(pids[small], pd[small], on[0][small], on[1][small], True, ctx)
    assert ok, why
    gt = brute_force_gt(X.astype(np.float32), labels, Q.astype(np.float32)[small], W[small], k, gu.metric_of(sfx))
    r_on, r_off = recall(gt, on[0][small], k), recall(gt, off[0][small], k)
    _record(f"rows {family} {sfx} d={d}: recall@10 of w <= L queries off {r_off:.4f} on {r_on:.4f}")
    assert r_on == 1.0
    # the inputs show something: without the option these queries get other rows
    assert (off[0][small] != on[0][small]).any(axis=1).sum() >= 1
    assert idx.set_exact_windows(0) == L


# ---- 2. rule edges ----------------------------------------------------------------------------------------------------------
def test_rule_edges(wa, gpu, cache, monkeypatch):
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.delenv("WANN_DENSE_ALWAYS", raising=False)
    sfx, d, n, k, L = "FloatEuclidian", 64, 20000, 10, 2000
    X, labels = _point_set(sfx, d, n, 5)
    rng = np.random.default_rng(9)
    nq = 64
    Q = _random_rows(sfx, rng, nq, d)
    w = np.tile(np.array([L, L + 1, 1, k - 1, 0, 700, 5000, 12]), nq // 8)
    a = rng.integers(1, n - 6000, nq)
    b = a + w
    a[4::16], b[4::16] = n + 100, n + 900     # beyond the label span (the others of this class are empty windows inside it)
    a[12:16], b[12:16] = -900, -100           # below it
    W = _pos_windows(a, b)
    idx = _index(wa, cache, "tree", sfx, X, labels, f"tree-{sfx}-{d}")
    fresh = _search(idx, "tree", Q, W, _qp(wa, k))
    c_fresh = idx.counters()
    assert idx.exact_window_counters() == ZERO
    assert idx.set_exact_windows(L) == 0 and idx.set_exact_windows(L) == L
    on = _search(idx, "tree", Q, W, _qp(wa, k))
    ec = idx.exact_window_counters()
    flagged = (w > 0) & (w <= L) & (a >= 0) & (b <= n)
    assert ec["queries"] == int(flagged.sum()) and ec["dense_queries"] == 0, ec
    assert ec["rows_scanned"] == int(w[flagged].sum()), ec
    assert _bits_equal(fresh, on, ~flagged)      # w = L + 1, wide, empty and outside windows: today's rows
    pi = wa.PrefilterIndexFloatEuclidian(X, labels)
    pids, pd = pi.batch_search(Q, W, nq, _qp(wa, k))
    for i in np.nonzero(flagged)[0]:
        m = min(k, int(w[i]))
        assert np.array_equal(on[1][i, :m].view(np.uint32), pd[i, :m].view(np.uint32)) and np.array_equal(on[0][i, :m], pids[i, :m]), i
        # w < k: the tree classes' padding (id 0, FLT_MAX)
        assert (on[0][i, m:] == 0).all() and (on[1][i, m:] == FLT_MAX).all(), (i, on[0][i], on[1][i])
    for i in np.nonzero((w == 0) | (a < 0) | (b > n))[0]:
        assert (on[0][i] == 0).all() and (on[1][i] == FLT_MAX).all()
    # L = 0 after L > 0: a fresh index
    assert idx.set_exact_windows(0) == L
    again = _search(idx, "tree", Q, W, _qp(wa, k))
    c_again = idx.counters()
    assert _bits_equal(fresh, again) and idx.exact_window_counters() == ZERO
    # (counters(): every field that counts work.  The rest of the struct is measured time -- device_ms, search_kernel_ms -- and
    # scheduling luck -- rounds, poll time-outs, look-aheads --, which differ between two calls of ONE index with the option off too)
    assert {f: c_again[f] for f in WORK} == {f: c_fresh[f] for f in WORK}
    with pytest.raises(Exception):
        idx.set_exact_windows(-1)
    assert idx.set_exact_windows(0) == 0


# ---- 3. methods -------------------------------------------------------------------------------------------------------------
def test_every_method_returns_the_same_exact_rows(wa, gpu, cache, monkeypatch):
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.delenv("WANN_DENSE_ALWAYS", raising=False)
    sfx, d, n, k, L, nq = "FloatEuclidian", 64, 20000, 10, 4096, 300
    X, labels = _point_set(sfx, d, n, 5)
    rng = np.random.default_rng(21)
    Q = _random_rows(sfx, rng, nq, d)
    w = rng.integers(300, 6001, nq)
    a = (rng.random(nq) * (n - w - 2)).astype(np.int64) + 1
    W = _pos_windows(a, a + w)
    small = w <= L
    idx = _index(wa, cache, "tree", sfx, X, labels, f"tree-{sfx}-{d}")
    rows = {}
    for method in ("optimized_postfilter", "fenwick", "three_split", "no_such_method"):
        assert idx.set_exact_windows(0) in (0, L)
        off = _search(idx, "tree", Q, W, _qp(wa, k), method)
        c_off = idx.counters()
        idx.set_exact_windows(L)
        on = _search(idx, "tree", Q, W, _qp(wa, k), method)
        c_on, ec = idx.counters(), idx.exact_window_counters()
        _record(f"methods {method}: {ec}, brute_rows off {c_off['brute_rows']} on {c_on['brute_rows']}")
        assert ec["queries"] == int(small.sum())
        assert _bits_equal(off, on, ~small), method       # w > L: the method's own rows
        if method != "optimized_postfilter":
            # the wide queries' fenwick / three_split covers have brute-forced ends: T_BRUTE tasks that are NOT exact windows
            assert c_on["brute_rows"] - ec["rows_scanned"] > 0, (method, c_on, ec)
        rows[method] = on
    for method, r in rows.items():
        assert _bits_equal(rows["optimized_postfilter"], r, small), method
    idx.set_exact_windows(0)


# ---- 4. the dense path is really used ------------------------------------------------------------------------------------------
USED_CASES = [("FloatEuclidian", 64), ("FloatMips", 256), ("Float16Mips", 100), ("UInt8Euclidian", 64)]  # narrow, wide, float16, bytes


@pytest.mark.parametrize("sfx,d", USED_CASES)
def test_dense_path_is_really_used(wa, gpu, cache, monkeypatch, sfx, d):
    """the inputs of test_cover_path_is_really_used on a tree index: uniform random rows, windows of 3 000 .. 12 000 of 40 000,
    at least 32 queries on every block"""
    n, nq, k, L = 40000, 2000, 10, 16384
    X, labels = _point_set(sfx, d, n, 3 + d)
    Q = _random_rows(sfx, np.random.default_rng(4 + d), nq, d)
    a, w = _used_batch(n, nq, 6 + d)
    W = _pos_windows(a, a + w)
    idx = _index(wa, cache, "tree", sfx, X, labels, f"used-{sfx}-{d}", cutoff=5000)
    idx.set_exact_windows(L)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    scan = _search(idx, "tree", Q, W, _qp(wa, k))
    es = idx.exact_window_counters()
    assert es["queries"] == nq and es["dense_queries"] == 0 and es["rows_scanned"] == int(w.sum()), es
    monkeypatch.delenv("WANN_NO_GEMM")
    dense = _search(idx, "tree", Q, W, _qp(wa, k))
    ed = idx.exact_window_counters()
    _record(f"used tree {sfx} d={d}: {ed}; scan-only rows_scanned {es['rows_scanned']}")
    assert ed["queries"] == nq and ed["dense_queries"] > nq // 2, ed
    assert ed["unproven"] <= nq // 10, ed
    assert ed["rows_scanned"] < es["rows_scanned"], (ed, es)
    assert _bits_equal(scan, dense)


# ---- 5. ties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (4, 32))
def test_ties_and_repeated_labels(oracle, wa, gpu, cache, monkeypatch, d):
    n, nq, k, L = 20000, 400, 10, 16384
    X = tie_heavy(n, d, 71 + d)
    Q = tie_queries(X, nq, 72 + d)
    labels = repeated_labels(n, 31, 150)
    rng = np.random.default_rng(73)
    s = np.sort(labels)
    W = np.zeros((nq, 2))
    for i in range(nq):  # ends are existing labels, inside runs of equal ones
        ww = int(rng.integers(1100, 9000))
        st = int(rng.integers(0, n - ww - 200))
        W[i] = (s[st], s[st + ww])
    idx = _index(wa, cache, "tree", "FloatEuclidian", X, labels, f"ties-{d}")
    idx.set_exact_windows(L)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    scan = _search(idx, "tree", Q, W, _qp(wa, k))
    es = idx.exact_window_counters()
    monkeypatch.delenv("WANN_NO_GEMM")
    dense = _search(idx, "tree", Q, W, _qp(wa, k))
    ed = idx.exact_window_counters()
    _record(f"ties d={d}: {ed}")
    assert es["queries"] == ed["queries"] > nq * 9 // 10 and ed["dense_queries"] > 0, (es, ed)
    assert _bits_equal(scan, dense)
    exact = np.searchsorted(s, W[:, 1].astype(np.float32), "left") - np.searchsorted(s, W[:, 0].astype(np.float32), "left") <= L
    oi = oracle.PrefilterIndexFloatEuclidian(X, labels)
    eids, edists = oi.batch_search(Q, W, nq, _qp(oracle, k))
    ctx = gu.RowContext(X, labels, Q[exact], W[exact], "l2", "prefilter")
    ok, why = gu.same_rows(eids[exact], edists[exact], dense[0][exact], dense[1][exact], True, ctx)
    assert ok, why


# ---- 6. a mixed batch through every call form --------------------------------------------------------------------------------
class _Exact(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in ("queries", "dense_queries", "unproven", "rescued", "passes", "rows_scanned")]


class _QP(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int64), ("beam_width", ctypes.c_int64), ("cut", ctypes.c_double), ("limit", ctypes.c_int64),
                ("degree_limit", ctypes.c_int64), ("final_beam_multiply", ctypes.c_int64), ("postfiltering_max_beam", ctypes.c_int64),
                ("has_ratio", ctypes.c_int32), ("ratio", ctypes.c_float), ("verbose", ctypes.c_int32)]


class _BP(ctypes.Structure):
    _fields_ = [("max_degree", ctypes.c_int64), ("limit", ctypes.c_int64), ("alpha", ctypes.c_double), ("cache_path", ctypes.c_char_p)]


def test_mixed_batch_every_call_form(wa, gpu, cache, monkeypatch):
    import torch
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    sfx, d, n, k, L = "FloatEuclidian", 64, 40000, 10, 16384
    X, labels = _point_set(sfx, d, n, 3 + d)
    nd = 1400
    a, w = _used_batch(n, nd, 8)
    rng = np.random.default_rng(12)
    a = np.concatenate([a, rng.integers(1, n - 2000, 200), rng.integers(1, n - 31000, 100), rng.integers(1, n, 40), np.full(20, n + 50)])
    w = np.concatenate([w, rng.integers(1, 1024, 200), rng.integers(17000, 30000, 100), np.zeros(40, dtype=np.int64), np.full(20, 500)])
    perm = rng.permutation(len(a))
    a, w = a[perm], w[perm]
    nq = len(a)
    Q = _random_rows(sfx, rng, nq, d)
    W = _pos_windows(a, a + w).astype(np.float32)
    flagged = (w > 0) & (w <= L) & (a + w <= n)
    idx = _index(wa, cache, "tree", sfx, X, labels, f"used-{sfx}-{d}", cutoff=5000)
    off = _search(idx, "tree", Q, W, _qp(wa, k))
    idx.set_exact_windows(L)
    host = _search(idx, "tree", Q, W, _qp(wa, k))
    ec = idx.exact_window_counters()
    _record(f"mixed batch: {ec}, counters {idx.counters()}")
    assert ec["queries"] == int(flagged.sum()) and ec["dense_queries"] > nd // 2 and ec["rows_scanned"] >= int(w[flagged & (w < 1024)].sum()), ec
    assert idx.counters()["beam_searches"] > 0
    assert _bits_equal(off, host, ~flagged) and (off[0][flagged] != host[0][flagged]).any()
    gt = brute_force_gt(X, labels, Q[flagged], W[flagged], k, "l2")
    assert recall(gt, host[0][flagged], k) == 1.0

    dev = torch.device("cuda:0")
    tq, tw = torch.from_numpy(Q).to(dev), torch.from_numpy(W).to(dev)

    def outputs(m):
        return torch.zeros((m, k), dtype=torch.int32, device=dev), torch.zeros((m, k), dtype=torch.float32, device=dev)

    def rows(ti, td):
        return ti.cpu().numpy().view(np.uint32), td.cpu().numpy()

    ti, td = outputs(nq)
    torch.cuda.synchronize()
    idx.batch_search_device(tq.data_ptr(), tw.data_ptr(), nq, 0, "optimized_postfilter", _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0)
    assert _bits_equal(host, rows(ti, td)) and idx.exact_window_counters() == ec
    tids = torch.arange(nq, dtype=torch.int64, device=dev)
    ti, td = outputs(nq)
    torch.cuda.synchronize()
    idx.batch_search_device_ids(tq.data_ptr(), tw.data_ptr(), nq, tids.data_ptr(), "optimized_postfilter", _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0)
    assert _bits_equal(host, rows(ti, td))
    # two lanes, two batches in flight: the whole batch and its second half (which keeps its query numbers)
    half = nq // 2
    outs = [outputs(nq), outputs(nq - half)]
    torch.cuda.synchronize()
    t0 = idx.batch_search_device_async(tq.data_ptr(), tw.data_ptr(), nq, 0, "optimized_postfilter", _qp(wa, k), outs[0][0].data_ptr(), outs[0][1].data_ptr(), 0)
    t1 = idx.batch_search_device_async(tq[half:].data_ptr(), tw[half:].data_ptr(), nq - half, half, "optimized_postfilter", _qp(wa, k),
                                       outs[1][0].data_ptr(), outs[1][1].data_ptr(), 0)
    idx.wait(t0)
    idx.wait(t1)
    assert _bits_equal(host, rows(*outs[0]))
    r1 = rows(*outs[1])
    assert np.array_equal(host[0][half:], r1[0]) and np.array_equal(host[1][half:].view(np.uint32), r1[1].view(np.uint32))
    idx.set_exact_windows(0)

    # the C ABI through ctypes: the same graphs from the cache, the same rows
    import rangefilteredann_amd
    lib = ctypes.CDLL(os.path.join(os.path.dirname(rangefilteredann_amd.__file__), "libwann.so"))
    lib.wann_index_create.restype = ctypes.c_void_p
    lib.wann_index_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.wann_index_destroy.argtypes = [ctypes.c_void_p]
    lib.wann_set_exact_windows.restype = ctypes.c_int64
    lib.wann_set_exact_windows.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.wann_get_exact_window_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Exact)]
    lib.wann_batch_search.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_char_p] + [ctypes.c_void_p] * 3
    assert lib.wann_abi_version() == 5
    Xc, lc, Qc, Wc = (np.ascontiguousarray(v) for v in (X, labels, Q, W))
    bp = _BP(32, 64, 1.0, os.path.join(cache, f"used-{sfx}-{d}", "").encode())
    h = lib.wann_index_create(3, 0, 0, Xc.ctypes.data, n, d, lc.ctypes.data, 5000, 2.0, 0.5, ctypes.byref(bp), 0, 4)
    assert h
    try:
        c = _Exact()
        assert lib.wann_get_exact_window_counters(h, ctypes.byref(c)) == 0 and c.queries == 0
        assert lib.wann_set_exact_windows(h, -1) == -1
        assert lib.wann_set_exact_windows(h, L) == 0 and lib.wann_set_exact_windows(h, L) == L
        qp = _QP(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, 0, 0.0, 0)
        ids = np.zeros((nq, k), dtype=np.uint32)
        dists = np.zeros((nq, k), dtype=np.float32)
        assert lib.wann_batch_search(h, Qc.ctypes.data, Wc.ctypes.data, nq, b"optimized_postfilter", ctypes.byref(qp), ids.ctypes.data, dists.ctypes.data) == 0
        assert lib.wann_get_exact_window_counters(h, ctypes.byref(c)) == 0
        assert {f: getattr(c, f) for f, _ in _Exact._fields_} == ec
        assert _bits_equal(host, (ids, dists))
    finally:
        lib.wann_index_destroy(h)
    # kinds without the option are refused with -WANN_ERR_UNSUPPORTED: PrefilterIndex (0), the stand-alone post filter (1: no
    # sorted labels; one small graph, R = 32) and the prefilter-leaf tree (2)
    small, small_labels = np.ascontiguousarray(X[:3000]), np.ascontiguousarray(labels[:3000])
    small_bp = _BP(32, 64, 1.0, b"")
    for kind in (0, 1, 2):
        t = lib.wann_index_create(kind, 0, 0, small.ctypes.data, 3000, d, small_labels.ctypes.data, 1000, 2.0, 0.5,
                                  ctypes.byref(small_bp) if kind == 1 else None, 0, 4)
        assert t
        try:
            assert lib.wann_set_exact_windows(t, 100) == -5 and lib.wann_set_exact_windows(t, 0) == -5
        finally:
            lib.wann_index_destroy(t)


# ---- 7. production mode ------------------------------------------------------------------------------------------------------
_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import rangefilteredann_amd, window_ann as wa
n, d, nq, k, L = 20000, 64, 200, 10, 16384
rng = np.random.default_rng(17)
x = rng.standard_normal((n + nq, d)).astype(np.float32)
x /= np.linalg.norm(x, axis=1, keepdims=True)
X, Q = x[:n], x[n:]
labels = rng.permutation(n).astype(np.float32)
w = rng.integers(2000, 12000, nq)
a = (rng.random(nq) * (n - w - 2)).astype(np.int64) + 1
W = np.stack([a - 0.5, a + w - 0.5], 1)
os.makedirs(sys.argv[2], exist_ok=True)
idx = wa.VamanaRangeFilterTreeIndexFloatEuclidian(X, labels, cutoff=5000, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, sys.argv[2]))
qp = wa.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False)
assert idx.set_exact_windows(L) == 0
ids, dists = idx.batch_search(Q, W, nq, "optimized_postfilter", qp)
ec = idx.exact_window_counters()
# 200 queries x <= 12 000 rows of 256 bytes: far below the 2 GiB of eligible rows the cover path asks of a batch
assert ec["queries"] == nq and ec["dense_queries"] == 0 and ec["rows_scanned"] == int(w.sum()), ec
pids, pd = wa.PrefilterIndexFloatEuclidian(X, labels).batch_search(Q, W, nq, qp)
assert np.array_equal(ids, pids) and np.array_equal(dists.view(np.uint32), pd.view(np.uint32))
print("production ok", ec)
"""


def test_production_mode_without_test_hooks(gpu, cache, tmp_path):
    env = dict(os.environ)
    env["WANN_TEST_HOOKS"] = "0"
    for name in list(env):
        if name.startswith("WANN_") and name not in ("WANN_TEST_HOOKS", "WANN_DEVICE"):
            del env[name]
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    out = subprocess.run([sys.executable, str(script), REPO, os.path.join(cache, "production", "")], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "production ok" in out.stdout, out.stdout[-1500:] + out.stderr[-1500:]
    _record(out.stdout.strip().splitlines()[-1])
