"""GPU: the wide call and the refined call's stop_k (include/wann.h WIDE ROWS / REFINED SEARCH).  A wide call
stops every doubling loop as the ordinary call at k = s does and keeps up to W entries of the frontier that loop returns.
What it must return is restated on the CPU oracle by wide_util.restate (one oracle call per level: tests/
test_wide_restatement.py is that util's own yardstick); ids and distance BITS are compared, and the work counters with the
engine's ordinary call at k = s.  Shapes: n = 3 000, d = 20, 200 queries -- a batch is a few milliseconds."""
import ctypes

import numpy as np
import pytest

import refine_util as ru
import wide_util as wu

pytestmark = pytest.mark.gpu
WORK = ("beam_searches", "hops", "dist_cmps")


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "ids", np.argwhere(got[0] != want[0])[:5].tolist())
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "distance bits")


def _work(idx):
    c = idx.counters()
    return [c[x] for x in WORK]


def _wide(idx, Q, W, nq, method, params, width):
    return idx.batch_search_wide(Q, W, nq, method, params, width) if method else idx.batch_search_wide(Q, W, nq, params, width)


@pytest.fixture(scope="module")
def pairs(wa, oracle, gpu, tmp_path_factory):
    """the float32 index of (kind, metric) on wide_util.data() and the oracle's index over the same graphs; built once"""
    cache = str(tmp_path_factory.mktemp("wide")) + "/"
    X, Q, labels, W = wu.data()
    built = {}

    def get(kind, metric):
        if (kind, metric) not in built:
            pi = getattr(wa, kind + "Float" + metric)(X, labels, **wu.kwargs_of(wa, kind, cache))
            oi = getattr(oracle, kind + "Float" + metric)(X, labels, **wu.kwargs_of(oracle, kind, cache))  # (opens the graphs the engine wrote)
            built[kind, metric] = (pi, oi)
        return built[kind, metric]

    return get


@pytest.fixture(scope="module")
def runs(wa, oracle, pairs):
    """one case of the parity grid: the wide rows and work counters, the ordinary rows at k = s and k = W with theirs, and the
    restatement; computed once per case and shared by the tests below"""
    done = {}

    def get(kind, method, metric, params):
        key = (kind, metric, params)
        if key not in done:
            s, width, B, mult, max_beam = params
            X, Q, labels, W = wu.data()
            pi, oi = pairs(kind, metric)
            wide = _wide(pi, Q, W, wu.NQ, method, wu.qp(wa, s, B, mult, max_beam), width)
            wide_work = _work(pi)
            at_s = wu.search(pi, Q, W, wu.NQ, method, wu.qp(wa, s, B, mult, max_beam))
            s_work = _work(pi)
            at_w = wu.search(pi, Q, W, wu.NQ, method, wu.qp(wa, width, B, mult, max_beam))
            want, _ = wu.restate(oracle, oi, Q, W, wu.NQ, method, s, width, B, mult, max_beam, ru.pad_id_of(kind))
            done[key] = dict(wide=wide, wide_work=wide_work, at_s=at_s, s_work=s_work, at_w=at_w, want=want)
        return done[key]

    return get


GRID = [pytest.param(kind, method, metric, params, id="%s-%s-s%d_W%d_B%d_x%d_max%d" % ((kind, metric) + params))
        for kind, method in wu.KINDS for metric in ("Euclidian", "Mips") for params in wu.PARAMS]


# ------------------------------------------------------------------------------------------
# 1. restatement parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,method,metric,params", GRID)
def test_restatement_parity(runs, kind, method, metric, params):
    s, width = params[:2]
    r = runs(kind, method, metric, params)
    ids, dists = r["wide"]
    assert ids.shape == (wu.NQ, width) and ids.dtype == np.uint32 and dists.dtype == np.float32
    cnt = ru.candidate_counts(ids, dists, ru.pad_id_of(kind))
    more = int((cnt > s).sum())
    differ = int(((ids != r["at_w"][0]) | (dists.view(np.uint32) != r["at_w"][1].view(np.uint32))).any(axis=1).sum())
    print(f"{kind}{metric} {params}: {more} rows hold more than s entries, {differ} differ from the ordinary call at k = W")
    _same(r["wide"], r["want"], (kind, metric, params))
    # conditions of the inputs (the oracle alone meets them: at least 60 and 90 in tests/test_wide_restatement.py): a call that
    # forwards to the ordinary one at k = s or at k = W fails here
    assert more >= 50 and differ >= 50
    _same((ids[:, :s], dists[:, :s]), r["at_s"], "prefix")


# ------------------------------------------------------------------------------------------
# 2. counters
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,method,metric,params", GRID)
def test_counters_equal_the_call_at_stop_k(runs, kind, method, metric, params):
    r = runs(kind, method, metric, params)
    assert r["wide_work"] == r["s_work"] and r["s_work"][0] > 0, (r["wide_work"], r["s_work"])


# ------------------------------------------------------------------------------------------
# 3. identity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,method", wu.KINDS + (("PrefilterIndex", ""), ("RangeFilterTreeIndex", "optimized_postfilter")))
def test_width_equal_to_k_is_the_ordinary_call(wa, pairs, tmp_path, kind, method):
    X, Q, labels, W = wu.data()
    if kind in ("PrefilterIndex", "RangeFilterTreeIndex"):  # no graph search: the wide call is the ordinary one at k = width
        pi = getattr(wa, kind + "FloatEuclidian")(X, labels, **({} if kind == "PrefilterIndex" else dict(cutoff=wu.CUTOFF, split_factor=2)))
        wide = _wide(pi, Q, W, wu.NQ, method, wu.qp(wa, 3, 8, 2, 10000), 40)
        _same(wide, wu.search(pi, Q, W, wu.NQ, method, wu.qp(wa, 40, 8, 2, 10000)), (kind, "k = width"))
    else:
        pi, _ = pairs(kind, "Euclidian")
    for k, B, mult in ((10, 16, 2), (64, 8, 1), (1, 4, 1)):
        params = wu.qp(wa, k, B, mult, 10000)
        plain = wu.search(pi, Q, W, wu.NQ, method, params)
        work = _work(pi)
        wide = _wide(pi, Q, W, wu.NQ, method, params, k)
        assert wide[0].tobytes() == plain[0].tobytes() and wide[1].tobytes() == plain[1].tobytes(), (kind, k)
        assert _work(pi) == work


@pytest.mark.parametrize("kind,method", wu.KINDS)
def test_stop_at_one_keep_1024(wa, oracle, pairs, kind, method):
    """(s, W) = (1, 1024): the first beam nearly always ends the loop, and the row is that beam's whole filtered frontier"""
    X, Q, labels, W = wu.data()
    pi, oi = pairs(kind, "Euclidian")
    s, width, B, mult, max_beam = 1, 1024, 8, 2, 10000
    wide = _wide(pi, Q, W, wu.NQ, method, wu.qp(wa, s, B, mult, max_beam), width)
    work = _work(pi)
    want, _ = wu.restate(oracle, oi, Q, W, wu.NQ, method, s, width, B, mult, max_beam, ru.pad_id_of(kind))
    _same(wide, want, kind)
    _same((wide[0][:, :1], wide[1][:, :1]), wu.search(pi, Q, W, wu.NQ, method, wu.qp(wa, s, B, mult, max_beam)), "prefix")
    assert _work(pi) == work
    cnt = ru.candidate_counts(wide[0], wide[1], ru.pad_id_of(kind))
    assert (cnt > 1).sum() >= 50 and cnt.max() < 1024  # (no row is full: a beam of 16 or 32, or a tiny window scanned exactly)


# ------------------------------------------------------------------------------------------
# 4. every chain mechanism
# ------------------------------------------------------------------------------------------
def _narrow(width, seed, nq=wu.NQ):
    rng = np.random.default_rng(seed)
    lo = rng.random(nq) * (1 - width)
    return np.stack([lo, lo + width], 1)


def _chain_case(wa, oracle, pairs, W, params, kind="PostfilterVamanaIndex", method=""):
    """a wide call (by default on the stand-alone post filter: its one partition is the whole set, so narrow windows mean long
    chains) against the restatement and the ordinary call's work counters; returns the wide call's counters and the rows' lengths"""
    s, width, B, mult, max_beam = params
    X, Q, labels, _ = wu.data()
    pi, oi = pairs(kind, "Euclidian")
    pad = ru.pad_id_of(kind)
    wide = _wide(pi, Q, W, wu.NQ, method, wu.qp(wa, s, B, mult, max_beam), width)
    c = pi.counters()
    want, _ = wu.restate(oracle, oi, Q, W, wu.NQ, method, s, width, B, mult, max_beam, pad)
    _same(wide, want, params)
    wu.search(pi, Q, W, wu.NQ, method, wu.qp(wa, s, B, mult, max_beam))
    assert _work(pi) == [c[x] for x in WORK]
    print(params, {x: c[x] for x in ("beam_searches", "spec_searches", "lookaheads_issued", "lookaheads_used", "deep_handoffs", "big_searches", "rounds")})
    return c, ru.candidate_counts(wide[0], wide[1], pad)


def test_chain_speculated_levels(wa, oracle, pairs):
    """windows of about 180 points across the median label: the tree's root partition (3 000 points) is the smallest that
    contains one, so its task is heavy (partition >= 8 x window) and k_route speculates its levels 8 .. 128, searched
    concurrently.  (The stand-alone post filter never speculates.)  On the oracle 58 of these 200 chains end below beam 128: the
    levels above the first one with >= s entries were speculation."""
    X, Q, labels, _ = wu.data()
    u = np.random.default_rng(6).uniform(0.2, 0.8, wu.NQ)
    mid = float(np.median(labels))
    W = np.stack([mid - u * 0.06, mid + (1 - u) * 0.06], 1)
    c, cnt = _chain_case(wa, oracle, pairs, W, (5, 20, 8, 1, 10000), "VamanaRangeFilterTreeIndex", "optimized_postfilter")
    assert c["spec_searches"] > 0 and (cnt > 5).sum() >= 50


def test_chain_lookaheads_or_handoffs(wa, oracle, pairs, monkeypatch):
    """chains that outgrow their speculated levels next to waiting pollers: windows of 150 points at (s = 10, first beam 16)
    are predicted to end at beam 256 and fail there about every second time; the chain then goes to a poller (beam 512 >= the
    hand-off beam) or has its next level searched ahead.  The 200-task launch counts as saturated through the test hook."""
    monkeypatch.setenv("WANN_DEEP_MIN_TASKS", "1")
    monkeypatch.setenv("WANN_LA_EAGER", "1")
    c, cnt = _chain_case(wa, oracle, pairs, _narrow(0.05, 4), (10, 40, 16, 1, 10000))
    assert c["lookaheads_issued"] > 0 or c["deep_handoffs"] > 0, c
    assert c["recovered_continuations"] == 0


def test_chain_ends_at_max_beam_with_a_short_row(wa, oracle, pairs):
    """windows of 12 points under postfiltering_max_beam = 100: the chain 4, 8, .. 64 cannot double again (128 >= 100), and the
    short row of the beam-64 level stands -- fewer than s entries, pads behind them"""
    c, cnt = _chain_case(wa, oracle, pairs, _narrow(0.004, 5), (3, 64, 4, 1, 100))
    assert (cnt < 3).sum() >= 50 and ((cnt > 0) & (cnt < 3)).any()
    assert c["beam_searches"] >= 5 * (cnt < 3).sum()  # (every short row searched all five levels)


# ------------------------------------------------------------------------------------------
# 5. fenwick and three_split
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ("Euclidian", "Mips"))
@pytest.mark.parametrize("method", ("fenwick", "three_split"))
def test_multi_bucket_methods(wa, oracle, pairs, method, metric):
    """several graph searches and two exact end scans per query, merged: the prefix property, the counters, and every entry an
    in-window point at its exact distance, rows ascending (continuous data: no ties)"""
    X, Q, labels, W = wu.data()
    pi, oi = pairs("VamanaRangeFilterTreeIndex", metric)
    dist = oracle.lib().orc_distance
    mcode = oracle.MIPS if metric == "Mips" else oracle.L2
    for s, width, B, mult, max_beam in wu.PARAMS:
        ids, dists = _wide(pi, Q, W, wu.NQ, method, wu.qp(wa, s, B, mult, max_beam), width)
        work = _work(pi)
        at_s = wu.search(pi, Q, W, wu.NQ, method, wu.qp(wa, s, B, mult, max_beam))
        assert _work(pi) == work and work[0] > 0
        _same((ids[:, :s], dists[:, :s]), at_s, (method, "prefix"))
        _same(at_s, wu.search(oi, Q, W, wu.NQ, method, wu.qp(oracle, s, B, mult, max_beam)), (method, "the oracle at k = s"))
        cnt = ru.candidate_counts(ids, dists, ru.PAD_SORTED)
        assert (cnt > s).sum() >= 50
        for q in range(wu.NQ):
            row, rd = ids[q, :cnt[q]].astype(np.int64), dists[q, :cnt[q]]
            assert (ids[q, cnt[q]:] == 0).all() and (dists[q, cnt[q]:] == ru.FLT_MAX).all()
            assert ((labels[row] >= np.float32(W[q, 0])) & (labels[row] <= np.float32(W[q, 1]))).all(), (method, q)
            assert (ru.fkey(rd)[1:] >= ru.fkey(rd)[:-1]).all(), (method, q)
            qp_ = Q[q].ctypes.data_as(ctypes.c_void_p)  # every non-pad entry of every query: one ctypes call each
            want = np.array([dist(mcode, X[i].ctypes.data_as(ctypes.c_void_p), qp_, wu.D) for i in row], dtype=np.float32)
            assert np.array_equal(rd.view(np.uint32), want.view(np.uint32)), (method, q)


def test_exact_windows_are_routed_by_the_width(wa, pairs):
    """set_exact_windows on a wide call: which windows are scanned exactly does not depend on k, so the graph searches and their
    counters stay the ordinary call's at k = s; whether the exact windows go through the matrix cores is decided on the row
    width (40 > 16: the scan), so gemm_queries is the ordinary call's at k = W, not at k = s.  The prefix property holds."""
    X, Q, labels, W = wu.data()
    W = W.copy()
    W[::2] = _narrow(0.4, 8)[::2]  # (about 1 200 points: wide enough for the dense path, below the limit)
    W[1::4] = _narrow(0.6, 9)[1::4]  # (about 1 800 points: above the limit, graph searched)
    pi, _ = pairs("VamanaRangeFilterTreeIndex", "Euclidian")
    s, width, B, mult, max_beam = wu.PARAMS[1]
    assert pi.set_exact_windows(1400) == 0
    try:
        wide = _wide(pi, Q, W, wu.NQ, "optimized_postfilter", wu.qp(wa, s, B, mult, max_beam), width)
        cw, ew = pi.counters(), pi.exact_window_counters()
        at_s = wu.search(pi, Q, W, wu.NQ, "optimized_postfilter", wu.qp(wa, s, B, mult, max_beam))
        cs, es = pi.counters(), pi.exact_window_counters()
        wu.search(pi, Q, W, wu.NQ, "optimized_postfilter", wu.qp(wa, width, B, mult, max_beam))
        cW = pi.counters()
    finally:
        pi.set_exact_windows(0)
    _same((wide[0][:, :s], wide[1][:, :s]), at_s, "prefix")
    assert [cw[x] for x in WORK] == [cs[x] for x in WORK] and cw["beam_searches"] > 0
    assert ew["queries"] == es["queries"] > 0 and ew["rows_scanned"] > 0
    assert cw["gemm_queries"] == cW["gemm_queries"] and cw["brute_rows"] == cW["brute_rows"]
    print("exact windows:", ew, es, cw["gemm_queries"], cs["gemm_queries"])


# ------------------------------------------------------------------------------------------
# 6. compact and byte units
# ------------------------------------------------------------------------------------------
def _rounder(wa, typ):
    return {"Float16": lambda x: x.astype(np.float16).astype(np.float32), "BFloat16": wa.bfloat16_round, "Float8": wa.float8_round,
            "UInt8": lambda x: np.clip(np.rint(x * 40 + 128), 0, 255).astype(np.float32)}[typ]


@pytest.mark.parametrize("typ", ("Float16", "BFloat16", "Float8", "UInt8", "half shadow rows"))
def test_every_unit(wa, gpu, tmp_path, typ):
    """the k_search units of the other element types and of the shadow rows: the wide rows of an index of that type equal the
    wide rows of the float32 index of the same (rounded) points -- the types' existing contract, now for the wide call"""
    X, Q, labels, W = wu.data(seed=2)
    rnd = _rounder(wa, "Float16" if typ == "half shadow rows" else typ)
    Xr, Qr = rnd(X), rnd(Q)
    kind, method = "VamanaRangeFilterTreeIndex", "optimized_postfilter"
    kw = wu.kwargs_of(wa, kind, str(tmp_path) + "/")
    f = getattr(wa, kind + "FloatEuclidian")(Xr, labels, **kw)
    if typ == "half shadow rows":
        h, elem = f, np.float32
        assert f.half_rows_bytes() > 0
    else:
        elem = np.uint8 if typ == "UInt8" else np.float32
        h = getattr(wa, kind + typ + "Euclidian")(Xr.astype(elem), labels, **kw)
    for s, width, B, mult, max_beam in wu.PARAMS:
        params = wu.qp(wa, s, B, mult, max_beam)
        if typ == "half shadow rows":
            assert f.set_half_rows(False) is False
        want = _wide(f, Qr, W, wu.NQ, method, params, width)
        work = _work(f)
        if typ == "half shadow rows":
            assert f.set_half_rows(True) is True
        got = _wide(h, Qr.astype(elem), W, wu.NQ, method, params, width)
        _same(got, want, (typ, s, width))
        assert _work(h) == work and work[0] > 0
        if typ == "half shadow rows":
            assert h.counters()["half_rows"] == 1
        cnt = ru.candidate_counts(got[0], got[1], ru.PAD_SORTED)
        assert (cnt > s).sum() >= 50
        _same((got[0][:, :s], got[1][:, :s]), wu.search(h, Qr.astype(elem), W, wu.NQ, method, params), (typ, "prefix"))


# ------------------------------------------------------------------------------------------
# 7. refined with stop_k
# ------------------------------------------------------------------------------------------
class _Device:
    """queries and windows of one batch on the device"""

    def __init__(self, Q, W):
        self.torch = pytest.importorskip("torch")
        self.dev = self.torch.device("cuda:0")
        self.nq = len(Q)
        self.tq = self.torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(self.dev)
        self.tw = self.torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).to(self.dev)

    def call(self, cols, fn):
        ti = self.torch.full((self.nq, cols), 7, dtype=self.torch.int32, device=self.dev)
        td = self.torch.full((self.nq, cols), -7.0, dtype=self.torch.float32, device=self.dev)
        self.torch.cuda.synchronize()
        fn(self.tq.data_ptr(), self.tw.data_ptr(), ti.data_ptr(), td.data_ptr())
        self.torch.cuda.synchronize()
        return ti.cpu().numpy().view(np.uint32), td.cpu().numpy()


@pytest.mark.parametrize("typ,kind,method,d", (("Float8", "VamanaRangeFilterTreeIndex", "optimized_postfilter", 36),
                                               ("BFloat16", "PostfilterVamanaIndex", "", 100),
                                               ("Float16", "SuperOptimizedPostfilterTreeIndex", "", 36)))
def test_refined_with_stop_k(wa, oracle, gpu, tmp_path, typ, kind, method, d):
    """the refined call at stop_k is the numpy re-rank (refine_util) of the wide row at (stop_k, width = refine_k); stop_k =
    refine_k is the refined call as it was; the search's counters are the ordinary call's at k = stop_k"""
    k, refine_k, B, mult = 10, 40, 16, 2
    X, Q, labels, W = wu.data(seed=3, d=d)
    scale = np.float32(16.0 if typ == "Float8" else 1.0)
    X, Q = X * scale, Q * scale
    idx = getattr(wa, kind + typ + "Euclidian")(_rounder(wa, typ)(X), labels, **wu.kwargs_of(wa, kind, str(tmp_path) + "/"))
    idx.set_refine_rows(X)
    dv = _Device(Q, W)
    pad = ru.pad_id_of(kind)
    old = dv.call(k, lambda q, w, i, t: idx.batch_search_device_refined(q, w, wu.NQ, 0, method, wu.qp(wa, k, B, mult, 10000), refine_k, i, t, 0))
    results = {}
    for stop_k in (k, 20, refine_k):
        cand = dv.call(refine_k, lambda q, w, i, t: idx.batch_search_device_wide(q, w, wu.NQ, 0, method, wu.qp(wa, stop_k, B, mult, 10000), refine_k, i, t, 0))
        want = ru.refine_reference(oracle, oracle.L2, X, Q, cand[0], cand[1], k, pad)
        got = dv.call(k, lambda q, w, i, t: idx.batch_search_device_refined(q, w, wu.NQ, 0, method, wu.qp(wa, k, B, mult, 10000), refine_k, i, t, 0,
                                                                            stop_k=stop_k))
        _same(got, want, (typ, kind, stop_k))
        work = _work(idx)
        assert idx.refine_counters()["refined_rows"] == ru.candidate_counts(cand[0], cand[1], pad).sum()
        dv.call(stop_k, lambda q, w, i, t: idx.batch_search_device(q, w, wu.NQ, 0, method, wu.qp(wa, stop_k, B, mult, 10000), i, t, 0))
        assert _work(idx) == work and work[0] > 0, stop_k
        results[stop_k] = (got, work)
    _same(results[refine_k][0], old, "stop_k = refine_k is the refined call without the argument")
    assert results[k][1][1] < results[refine_k][1][1]  # fewer hops: the search at k, not the one at refine_k
    host = idx.batch_search_refined(Q, W, wu.NQ, method, wu.qp(wa, k, B, mult, 10000), refine_k, stop_k=20)
    _same(host, results[20][0], "host form")


# ------------------------------------------------------------------------------------------
# 8. refusals
# ------------------------------------------------------------------------------------------
def test_refusals(wa, pairs, gpu, tmp_path):
    X, Q, labels, W = wu.data()
    pi, _ = pairs("VamanaRangeFilterTreeIndex", "Euclidian")
    method, k = "optimized_postfilter", 10
    good = wu.qp(wa, k, 16, 2, 10000)
    verbose = wa.QueryParams(k, 16, 1.35, 10_000_000, 10_000, 2, 10000, None, True)
    _wide(pi, Q, W, wu.NQ, method, good, 40)
    before = pi.counters()
    dv = _Device(Q, W)
    for width in (k - 1, 0, -3, 1025):
        with pytest.raises(RuntimeError, match="k <= width <= 1024"):
            _wide(pi, Q, W, wu.NQ, method, good, width)
        with pytest.raises(RuntimeError, match="k <= width <= 1024"):
            dv.call(8, lambda q, w, i, t: pi.batch_search_device_wide(q, w, wu.NQ, 0, method, good, width, i, t, 0))
    with pytest.raises(RuntimeError, match="k <= width <= 1024"):
        _wide(pi, Q, W, wu.NQ, method, wu.qp(wa, 0, 16, 2, 10000), 40)
    with pytest.raises(RuntimeError, match="verbose"):
        _wide(pi, Q, W, wu.NQ, method, verbose, 40)
    with pytest.raises(RuntimeError, match="verbose"):
        dv.call(40, lambda q, w, i, t: pi.batch_search_device_wide(q, w, wu.NQ, 0, method, verbose, 40, i, t, 0))
    assert pi.counters() == before  # none of these launched anything
    # the refined call's stop_k
    X8 = X * np.float32(16)
    idx = wa.PrefilterIndexFloat8Euclidian(wa.float8_round(X8), labels)
    idx.set_refine_rows(X8)
    idx.batch_search_refined(Q, W, wu.NQ, "", good, 40, stop_k=20)
    before = (idx.counters(), idx.refine_counters())
    for stop_k in (k - 1, 41, 0, -1):
        with pytest.raises(RuntimeError, match="k <= stop_k <= refine_k"):
            idx.batch_search_refined(Q, W, wu.NQ, "", good, 40, stop_k=stop_k)
        with pytest.raises(RuntimeError, match="k <= stop_k <= refine_k"):
            dv.call(k, lambda q, w, i, t: idx.batch_search_device_refined(q, w, wu.NQ, 0, "", good, 40, i, t, 0, stop_k=stop_k))
    with pytest.raises(RuntimeError, match="verbose"):
        idx.batch_search_refined(Q, W, wu.NQ, "", verbose, 40, stop_k=20)
    with pytest.raises(RuntimeError, match="verbose"):
        dv.call(k, lambda q, w, i, t: idx.batch_search_device_refined(q, w, wu.NQ, 0, "", verbose, 40, i, t, 0, stop_k=20))
    assert (idx.counters(), idx.refine_counters()) == before
    # the C ABI answers a null index with the negative code, as the refined calls do
    import rangefilteredann_amd
    lib = ctypes.CDLL(rangefilteredann_amd.lib_path())
    lib.wann_batch_search_wide.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 2
    assert lib.wann_batch_search_wide(None, None, None, 0, b"", None, 40, None, None) == -1
