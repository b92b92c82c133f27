"""GPU: the refined search (include/wann.h REFINED SEARCH).  A float16 / bfloat16 / float8 index is built from
the ROUNDED points of a real-valued set, the unrounded float32 points are its refine rows, and a refined call must return --
ids and distance BITS -- what refine_util.refine_reference makes of the same index's ordinary call at k = refine_k: every
candidate re-scored against its full-precision row in the float32 index's arithmetic (the oracle's distance()), the best k
under (distance, id), pads behind them.  A kernel that does nothing cannot pass: the rounded points' distances differ in bits."""
import numpy as np
import pytest

import refine_util as ru
from util import distinct_labels, repeated_labels, windows

pytestmark = pytest.mark.gpu
N, NQ = 3000, 96
OPS = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads", "spec_searches", "gemm_queries", "gemm_unproven", "gemm_rescued")
SCALE = {"Float16": 1.0, "BFloat16": 1.0, "Float8": 16.0}  # a power of two that spreads the set over float8's range (|x| < 448)
KINDS = {"PrefilterIndex": dict(), "PostfilterVamanaIndex": dict(), "RangeFilterTreeIndex": dict(cutoff=300, split_factor=2),
         "VamanaRangeFilterTreeIndex": dict(cutoff=300, split_factor=2),
         "SuperOptimizedPostfilterTreeIndex": dict(cutoff=300, split_factor=2, shift_factor=0.5)}


def _qp(mod, k, beam=40, mult=2):
    return mod.QueryParams(k, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)


def _round(wa, typ, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x.astype(np.float16).astype(np.float32) if typ == "Float16" else wa.bfloat16_round(x) if typ == "BFloat16" else wa.float8_round(x)


def _data(wa, typ, n, d, seed, nq=NQ):
    """real-valued points and fp32 queries (normals x 3.1 + 0.37, scaled into range): neither is made of values of the compact type"""
    rng = np.random.default_rng(seed)
    X = ((rng.standard_normal((n, d)) * 3.1 + 0.37) * SCALE[typ]).astype(np.float32)
    Q = ((rng.standard_normal((nq, d)) * 3.1 + 0.37) * SCALE[typ]).astype(np.float32)
    assert np.abs(X).max() < 448 and (_round(wa, typ, X) != X).mean() > 0.9 and (_round(wa, typ, Q) != Q).mean() > 0.9
    return X, Q


def _index(wa, kind, typ, metric, X, labels, tmp_path, store=True):
    """the index of the ROUNDED points; its refine rows are the unrounded ones"""
    kw = dict(KINDS[kind])
    if kind != "PrefilterIndex" and kind != "RangeFilterTreeIndex":
        kw["build_params"] = wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/")
    idx = getattr(wa, kind + typ + metric)(_round(wa, typ, X), labels, **kw)
    if store:
        idx.set_refine_rows(X)
    return idx


class _Device:
    """queries and windows of one batch on the device; ordinary and refined device-buffer calls on them"""

    def __init__(self, Q, W):
        self.torch = pytest.importorskip("torch")
        self.dev = self.torch.device("cuda:0")
        self.nq = len(Q)
        self.tq = self.torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(self.dev)
        self.tw = self.torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).to(self.dev)

    def _out(self, k):
        ti = self.torch.full((self.nq, k), 7, dtype=self.torch.int32, device=self.dev)
        td = self.torch.full((self.nq, k), -7.0, dtype=self.torch.float32, device=self.dev)
        self.torch.cuda.synchronize()
        return ti, td

    def _back(self, ti, td):
        self.torch.cuda.synchronize()
        return ti.cpu().numpy().view(np.uint32), td.cpu().numpy()

    def search(self, wa, idx, k, method=""):
        ti, td = self._out(k)
        idx.batch_search_device(self.tq.data_ptr(), self.tw.data_ptr(), self.nq, 0, method, _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0)
        return self._back(ti, td)

    def refined(self, wa, idx, k, refine_k, method=""):
        ti, td = self._out(k)
        idx.batch_search_device_refined(self.tq.data_ptr(), self.tw.data_ptr(), self.nq, 0, method, _qp(wa, k), refine_k, ti.data_ptr(),
                                        td.data_ptr(), 0)
        return self._back(ti, td)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "ids", np.argwhere(got[0] != want[0])[:5].tolist())
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "distance bits")


def _check(oracle, wa, idx, dv, X, Q, metric, kind, k, refine_k, method=""):
    """one refined call against the reference made from the same index's ordinary call at k = refine_k; returns (candidate rows,
    refined rows)"""
    pad = ru.pad_id_of(kind)
    cand = dv.search(wa, idx, refine_k, method)
    want = ru.refine_reference(oracle, oracle.MIPS if metric == "Mips" else oracle.L2, X, Q, cand[0], cand[1], k, pad)
    got = dv.refined(wa, idx, k, refine_k, method)
    _same(got, want, (kind, metric, k, refine_k, method))
    return cand, got


def _mixed_windows(labels, nq, seed, fractions=(-4, -3, -2, -1)):
    Ws = [windows(labels, nq, p, seed + p) for p in fractions]
    return np.concatenate([w[i::len(Ws)] for i, w in enumerate(Ws)])[:nq]


def _windows_of(labels, nq, widths, seed):
    """windows that hold exactly widths[i % len] points of the label order (distinct labels): both ends lie between two labels"""
    rng = np.random.default_rng(seed)
    s = np.sort(labels).astype(np.float64)
    n = len(s)
    out = np.zeros((nq, 2))
    w = np.array([widths[i % len(widths)] for i in range(nq)])
    for i in range(nq):
        st = int(rng.integers(1, n - w[i] - 1))
        out[i] = ((s[st - 1] + s[st]) / 2, (s[st + w[i] - 1] + s[st + w[i]]) / 2)
    return out, w


# ------------------------------------------------------------------------------------------
# 1. the exact kind, every fetch shape
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (4, 36, 100, 260))  # below one 16-float group, no multiple of 16, the common case, several lane passes
@pytest.mark.parametrize("metric", ("Euclidian", "Mips"))
@pytest.mark.parametrize("typ", ("Float16", "BFloat16", "Float8"))
def test_exact_kind_every_fetch_shape(oracle, wa, gpu, tmp_path, typ, metric, d):
    for n, pairs in ((N, ((10, 10), (10, 40), (10, 64), (10, 65), (64, 128))), (4096, ((1, 1024),))):  # 65 crosses the 64-candidate chunk
        X, Q = _data(wa, typ, n, d, 100 + d)
        labels = distinct_labels(n, 5)
        idx = _index(wa, "PrefilterIndex", typ, metric, X, labels, tmp_path)
        dv = _Device(Q, _mixed_windows(labels, NQ, 40))
        for k, refine_k in pairs:
            cand, got = _check(oracle, wa, idx, dv, X, Q, metric, "PrefilterIndex", k, refine_k)
            assert idx.refine_counters()["refined_rows"] == ru.candidate_counts(cand[0], cand[1], ru.PAD_RAW).sum()
            if refine_k > k:  # the rounded points' distances are not the refined ones: the kernel did something
                assert not np.array_equal(got[1].view(np.uint32), cand[1][:, :k].view(np.uint32))


# ------------------------------------------------------------------------------------------
# 2. pads
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ,metric", (("Float8", "Euclidian"), ("BFloat16", "Mips")))
@pytest.mark.parametrize("kind", ("PostfilterVamanaIndex", "RangeFilterTreeIndex"))
def test_pads(oracle, wa, gpu, tmp_path, kind, typ, metric):
    """windows of 0, 3 (< k) and 25 (k < 25 < refine_k) points among full ones: a pad suffix of exactly the expected length"""
    k, refine_k, d = 10, 40, 36
    X, Q = _data(wa, typ, N, d, 7)
    labels = distinct_labels(N, 6)
    W, width = _windows_of(labels, NQ, (0, 3, 400, 25, 200, 3, 0, 25, 1500), 3)
    idx = _index(wa, kind, typ, metric, X, labels, tmp_path)
    dv = _Device(Q, W)
    cand, (ids, dists) = _check(oracle, wa, idx, dv, X, Q, metric, kind, k, refine_k, "optimized_postfilter")
    pad = ru.pad_id_of(kind)
    assert pad == (0 if kind == "RangeFilterTreeIndex" else 0xFFFFFFFF)
    cnt = ru.candidate_counts(cand[0], cand[1], pad)
    if kind == "RangeFilterTreeIndex":  # exact leaves: every point of a window is a candidate
        assert np.array_equal(cnt, np.minimum(width, refine_k))
    else:
        assert (cnt <= np.minimum(width, refine_k)).all() and (cnt[width >= 200] == refine_k).all()
    assert {0, 3, 25} <= set(np.minimum(width, refine_k).tolist()) and (cnt[width == 0] == 0).all() and (cnt > k).any()
    is_pad = (ids == np.uint32(pad)) & (dists == ru.FLT_MAX)
    assert np.array_equal(is_pad.sum(axis=1), k - np.minimum(cnt, k))
    assert np.array_equal(is_pad, np.arange(k)[None, :] >= np.minimum(cnt, k)[:, None])  # a suffix
    assert (dists[~is_pad] < ru.FLT_MAX).all()
    assert idx.refine_counters() == dict(idx.refine_counters(), refined_queries=NQ, refined_rows=int(cnt.sum()))


# ------------------------------------------------------------------------------------------
# 3. every kind and method
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ,metric", (("Float8", "Euclidian"), ("Float8", "Mips"), ("BFloat16", "Euclidian"), ("BFloat16", "Mips")))
@pytest.mark.parametrize("kind", ("PostfilterVamanaIndex", "RangeFilterTreeIndex", "VamanaRangeFilterTreeIndex", "SuperOptimizedPostfilterTreeIndex"))
def test_every_kind_and_method(oracle, wa, gpu, tmp_path, kind, typ, metric):
    k, refine_k, d = 10, 40, 36
    X, Q = _data(wa, typ, N, d, 11)
    labels = distinct_labels(N, 8)
    idx = _index(wa, kind, typ, metric, X, labels, tmp_path)
    methods = ("optimized_postfilter", "fenwick", "three_split") if kind == "VamanaRangeFilterTreeIndex" else ("optimized_postfilter",)
    pad = ru.pad_id_of(kind)
    for method in methods:
        for p in (-5, -4, -3, -2, -1):
            dv = _Device(Q, windows(labels, NQ, p, 20 + p))
            cand = dv.search(wa, idx, refine_k, method)
            ordinary = idx.counters()
            want = ru.refine_reference(oracle, oracle.MIPS if metric == "Mips" else oracle.L2, X, Q, cand[0], cand[1], k, pad)
            got = dv.refined(wa, idx, k, refine_k, method)
            _same(got, want, (kind, typ, metric, method, p))
            after = idx.counters()
            assert [after[x] for x in OPS] == [ordinary[x] for x in OPS], (method, p, after, ordinary)
            rc = idx.refine_counters()
            assert rc["refined_rows"] == ru.candidate_counts(cand[0], cand[1], pad).sum() and rc["refined_queries"] == NQ and rc["refine_ms"] > 0


# ------------------------------------------------------------------------------------------
# 4. ties
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ,metric", (("BFloat16", "Euclidian"), ("Float8", "Mips")))
@pytest.mark.parametrize("kind,methods", (("PrefilterIndex", ("",)), ("VamanaRangeFilterTreeIndex", ("fenwick", "three_split"))))
def test_ties(oracle, wa, gpu, tmp_path, kind, methods, typ, metric):
    """store rows of small integers, every row present twice: equal refined distances, ordered by id.  Labels repeat (runs of
    about 20 points share one), so the side searches of three_split admit points its centre search returns too: ids occur twice
    among the candidates (checked for this seed on the CPU oracle: 48 of the 96 queries), and such an id stays twice.  (fenwick
    covers its sides by position and repeats no id on this data.)"""
    k, refine_k, d = 10, 40, 6
    rng = np.random.default_rng(19)
    A = rng.integers(0, 12, (N // 2, d)).astype(np.float32)
    X = np.concatenate([A, A])[rng.permutation(N)]
    Q = rng.integers(0, 12, (NQ, d)).astype(np.float32)
    assert np.array_equal(_round(wa, typ, X), X)
    labels = repeated_labels(N, 4, 150)
    kw = dict(KINDS[kind])
    if kind != "PrefilterIndex":
        kw["build_params"] = wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/")
    idx = getattr(wa, kind + typ + metric)(X, labels, **kw)
    idx.set_refine_rows(X)
    dv = _Device(Q, _mixed_windows(labels, NQ, 9, (-3, -2, -1)))
    for method in methods:
        cand, (ids, dists) = _check(oracle, wa, idx, dv, X, Q, metric, kind, k, refine_k, method)
        tied = dists[:, 1:] == dists[:, :-1]
        assert tied.sum() > NQ  # many equal distances ...
        assert (ids[:, 1:][tied].astype(np.int64) >= ids[:, :-1][tied].astype(np.int64)).all()  # ... in id order
        dup = sum(len(r) - len(set(r.tolist())) for r in cand[0])
        print(f"{kind} {method}: {int(tied.sum())} tied neighbours, {dup} repeated ids among the candidates")
        if method == "three_split":
            assert dup > 0  # duplicate ids reached the kernel ...
            kept = [r[dd < ru.FLT_MAX] for r, dd in zip(ids, dists)]
            assert sum(len(r) - len(set(r.tolist())) for r in kept) > 0  # ... and some of them are among the best k: they stayed


# ------------------------------------------------------------------------------------------
# 5. refinement can only help an exact scan
# ------------------------------------------------------------------------------------------
def test_refinement_only_helps_an_exact_scan(oracle, wa, gpu, tmp_path):
    """PrefilterIndexFloat8Euclidian: the refined key order is the ground truth's, so per query the refined row holds at least as
    many of the true top 10 as the unrefined one -- and more for some query (checked for this seed with numpy on the rounded
    points).  Fails if the kernel scores the wrong row or the wrong query."""
    k, refine_k, d = 10, 40, 36
    X, Q = _data(wa, "Float8", N, d, 23)
    labels = distinct_labels(N, 2)
    W, width = _windows_of(labels, NQ, (375, 200, 750), 5)
    idx = _index(wa, "PrefilterIndex", "Float8", "Euclidian", X, labels, tmp_path)
    dv = _Device(Q, W)
    plain = dv.search(wa, idx, k)
    got = dv.refined(wa, idx, k, refine_k)
    dist = oracle.lib().orc_distance
    import ctypes
    better = 0
    for q in range(NQ):
        inside = np.nonzero((labels.astype(np.float64) > W[q, 0]) & (labels.astype(np.float64) < W[q, 1]))[0]
        assert len(inside) == width[q]
        qp = Q[q].ctypes.data_as(ctypes.c_void_p)
        td = np.array([dist(oracle.L2, X[i].ctypes.data_as(ctypes.c_void_p), qp, d) for i in inside], dtype=np.float32)
        gt = set(inside[np.lexsort((inside, ru.fkey(td)))[:k]].tolist())
        r, u = len(gt & set(got[0][q].tolist())), len(gt & set(plain[0][q].tolist()))
        assert r >= u, (q, r, u)
        better += r > u
    assert better >= 1


# ------------------------------------------------------------------------------------------
# 6. nothing else moved
# ------------------------------------------------------------------------------------------
def test_nothing_else_moved(wa, gpu, tmp_path):
    k, d = 10, 36
    X, Q = _data(wa, "BFloat16", N, d, 31)
    labels = distinct_labels(N, 3)
    idx = _index(wa, "VamanaRangeFilterTreeIndex", "BFloat16", "Euclidian", X, labels, tmp_path, store=False)
    W = _mixed_windows(labels, NQ, 12)
    dv = _Device(Q, W)
    Qh = wa.bfloat16_round(Q)
    assert idx.refine_rows_bytes() == 0
    bytes0 = idx.device_bytes()
    host0 = idx.batch_search(Qh, W, NQ, "optimized_postfilter", _qp(wa, k))
    dev0 = dv.search(wa, idx, k, "optimized_postfilter")
    idx.set_refine_rows(X)
    assert idx.refine_rows_bytes() == N * 4 * 16 * -(-d // 16) and idx.device_bytes() == bytes0
    _same(idx.batch_search(Qh, W, NQ, "optimized_postfilter", _qp(wa, k)), host0, "host")
    _same(dv.search(wa, idx, k, "optimized_postfilter"), dev0, "device")
    dv.refined(wa, idx, k, 40, "optimized_postfilter")
    _same(dv.search(wa, idx, k, "optimized_postfilter"), dev0, "device, after a refined call")
    idx.set_refine_rows(X.astype(np.float64))  # (any array numpy casts to float32; a second call replaces the store)
    assert idx.refine_rows_bytes() == N * 4 * 16 * -(-d // 16)
    idx.set_refine_rows(None)
    assert idx.refine_rows_bytes() == 0 and idx.device_bytes() == bytes0
    with pytest.raises(RuntimeError, match="refine rows"):
        idx.batch_search_refined(Q, W, NQ, "optimized_postfilter", _qp(wa, k), 40)


# ------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------
def test_refusals(wa, gpu, tmp_path):
    k, d = 10, 36
    X, Q = _data(wa, "Float8", N, d, 37)
    labels = distinct_labels(N, 1)
    W = _mixed_windows(labels, NQ, 14)
    for cls, pts in ((wa.PrefilterIndexFloatEuclidian, X), (wa.PrefilterIndexUInt8Euclidian, np.clip(X, 0, 255).astype(np.uint8))):
        other = cls(pts, labels)
        with pytest.raises(RuntimeError, match="float16 / bfloat16 / float8"):
            other.set_refine_rows(X)
        assert other.refine_rows_bytes() == 0
    idx = _index(wa, "PrefilterIndex", "Float8", "Euclidian", X, labels, tmp_path)
    size = idx.refine_rows_bytes()
    idx.batch_search_refined(Q, W, NQ, "", _qp(wa, k), 40)
    before = (idx.counters(), idx.refine_counters())
    for bad, why in ((X[:-1], "points"), (X[:, :-1], "points")):  # wrong n, wrong d
        with pytest.raises(RuntimeError, match=why):
            idx.set_refine_rows(bad)
    for v in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[17, 5] = v
        Y[400, 0] = v
        with pytest.raises(RuntimeError, match="row 17"):
            idx.set_refine_rows(Y)
    with pytest.raises(RuntimeError):
        idx.set_refine_rows(X[0])  # not 2-dimensional
    assert idx.refine_rows_bytes() == size  # the store in place was kept
    dv = _Device(Q, W)
    for refine_k in (k - 1, 1025, 0):
        with pytest.raises(RuntimeError, match="refine_k"):
            idx.batch_search_refined(Q, W, NQ, "", _qp(wa, k), refine_k)
        with pytest.raises(RuntimeError, match="refine_k"):
            dv.refined(wa, idx, k, refine_k)
    idx.set_refine_rows(None)
    with pytest.raises(RuntimeError, match="no refine rows"):
        dv.refined(wa, idx, k, 40)
    with pytest.raises(RuntimeError, match="no refine rows"):
        idx.batch_search_refined(Q, W, NQ, "", _qp(wa, k), 40)
    assert (idx.counters(), idx.refine_counters()) == before  # none of these launched anything


# ------------------------------------------------------------------------------------------
# 8. the host form
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,typ,metric", (("PrefilterIndex", "Float16", "Mips"), ("VamanaRangeFilterTreeIndex", "Float8", "Euclidian")))
def test_host_form_equals_device_form(wa, gpu, tmp_path, kind, typ, metric):
    k, refine_k, d = 10, 40, 100
    X, Q = _data(wa, typ, N, d, 41)
    labels = distinct_labels(N, 7)
    W = _mixed_windows(labels, NQ, 16)
    idx = _index(wa, kind, typ, metric, X, labels, tmp_path)
    dev = _Device(Q, W).refined(wa, idx, k, refine_k, "optimized_postfilter")
    host = idx.batch_search_refined(Q, W, NQ, "optimized_postfilter", _qp(wa, k), refine_k)
    assert host[0].dtype == np.uint32 and host[1].dtype == np.float32 and host[0].shape == (NQ, k)
    _same(host, dev, (kind, typ, metric))
    host64 = idx.batch_search_refined(Q.astype(np.float64), W, NQ, "optimized_postfilter", _qp(wa, k), refine_k)  # cast to float32, not rounded further
    _same(host64, dev, "float64 queries")
