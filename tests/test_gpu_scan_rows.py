"""GPU: the exact scans of a float32 index read its shadow rows (include/wann.h, wann_set_scan_rows).  With the switch on,
k_brute reads the copy that the same batch's beam searches read -- the one-byte rows if set_byte_rows is on, else the half rows
-- widens every element exactly and runs the float32 scan's arithmetic in its order.  So every batch is run three ways (switch
off; on with half rows; on with one-byte rows) and ids, distance BITS and the work counters must be equal: no tolerance anywhere.

The points are integers 0 .. 255 (+0.0 only: both copies exist); the queries are NOT integers, so their fp32 sums depend on the
evaluation order and equal distance bits show that the order was kept.  n = 6 037 is no multiple of 64: a scan that ends on the
last row ends in the middle of a 64-row pass, and the copies end with that row."""
import numpy as np
import pytest

import golden_util as gu
from util import distinct_labels, sift_like, tie_heavy, tie_queries, windows

pytestmark = pytest.mark.gpu
N, NQ = 6037, 200
WORK = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads")
LEGS = (("off", 0), ("half", 1), ("byte", 2))  # (leg, what counters()["scan_rows"] reports for a batch that scans)
WIDTHS = (1, 63, 64, 65, 127, 129)


def _qp(mod, k=10, beam=20, mult=1):
    return mod.QueryParams(k, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)


def _sift(d, seed):
    g = sift_like(N, d, seed)
    X, Q = g(N) + np.float32(0), g(NQ)  # (+ 0: numpy's clip keeps the -0.0 that rint makes, and the one-byte rule is on bits)
    assert not np.signbit(X).any() and X.dtype == np.float32 and X.min() >= 0 and X.max() <= 255 and (X >= 128).any()
    Q = (Q + np.random.default_rng(seed + 1000).random(Q.shape, dtype=np.float32)).astype(np.float32)
    assert not np.array_equal(Q, np.rint(Q))
    return X, Q


def _ties(seed):
    X = tie_heavy(N, 6, seed)  # (d = 6, values below 12, 15 % of the rows copies of other rows: equal keys are ordered by id)
    return X, tie_queries(X, NQ, seed + 1)


TREE, SUPER = "VamanaRangeFilterTreeIndexFloatEuclidian", "SuperOptimizedPostfilterTreeIndexFloatMips"
# d = 128: 16 blocks, the two-row routine; d = 20: three blocks ("last block first"), a 20-byte row in a 64-byte pitch, a half row
# of 40 bytes in 64; d = 100 under the inner product: the 13-step routine; d = 200: the routine without a compile-time block count
CASES = {
    "sift128_l2_tree": (TREE, lambda: _sift(128, 61), dict(cutoff=1000, split_factor=2)),
    "sift20_l2_tree": (TREE, lambda: _sift(20, 62), dict(cutoff=1000, split_factor=2)),
    "sift100_mips_super": (SUPER, lambda: _sift(100, 63), dict(cutoff=400, split_factor=2, shift_factor=0.5)),
    "sift200_l2_tree": (TREE, lambda: _sift(200, 64), dict(cutoff=1000, split_factor=2)),
    "ties6_l2_tree": (TREE, lambda: _ties(65), dict(cutoff=1000, split_factor=2)),
}


class Built:
    def __init__(self, wa, torch, cls, X, Q, kw, cache=""):
        self.labels = distinct_labels(N, 9)
        self.sorted = np.sort(self.labels)
        self.cls, self.kw, self.cache, self.X, self.Q = cls, kw, cache, X, Q
        self.idx = getattr(wa, cls)(X, self.labels, build_params=wa.BuildParams(32, 64, 1.0, cache), **kw)
        self.tree = cls.startswith("VamanaRangeFilterTreeIndex")
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.tq = torch.from_numpy(Q).to(self.dev)

    def leg(self, which):
        """the rows the next batches' scans read: the index's own (switch off), the half rows, the one-byte rows"""
        idx = self.idx
        assert idx.set_half_rows(True) is True
        assert idx.set_byte_rows(which == "byte") is (which == "byte")
        assert idx.set_scan_rows(which != "off") is (which != "off")
        assert idx.scan_rows() is (which != "off")

    def rank_windows(self, a, b):
        """label windows that hold exactly rows [a, b) of the sorted order under the tree's half-open rule"""
        s = self.sorted
        hi = [s[x] if x < N else s[-1] + 1 for x in b]
        return np.stack([s[np.asarray(a)], np.asarray(hi)], 1).astype(np.float64)

    def call(self, form, W, method, qp, nq, k):
        """rows (ids, distance bits) and counters of one batch of the first nq queries"""
        idx, torch = self.idx, self.torch
        if form == "host":
            a = (method,) if self.tree else ()
            ids, dists = idx.batch_search(self.Q[:nq], W, nq, *a, qp)
            return ids.view(np.uint32).copy(), dists.view(np.uint32).copy(), idx.counters()
        tw = torch.from_numpy(np.asarray(W, dtype=np.float32)).to(self.dev)
        ti = torch.zeros((nq, k), dtype=torch.int32, device=self.dev)
        td = torch.zeros((nq, k), dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize()
        idx.batch_search_device(self.tq.data_ptr(), tw.data_ptr(), nq, 0, method if self.tree else "", qp, ti.data_ptr(), td.data_ptr(), 0)
        return ti.cpu().numpy().view(np.uint32), td.cpu().numpy().view(np.uint32), idx.counters()

    def three_ways(self, wa, W, method="optimized_postfilter", k=10, beam=20, exact=0, form="host", what=None):
        """the same batch with the switch off, on with the half rows, on with the one-byte rows: equal rows, equal work, the store
        each scan reports, and a scan that scored rows.  Returns the switch-off leg."""
        W = np.asarray(W)
        nq = len(W)
        rows = {}
        try:
            if exact:
                assert self.idx.set_exact_windows(exact) == 0
            for leg, code in LEGS:
                self.leg(leg)
                rows[leg] = r = self.call(form, W, method, _qp(wa, k, beam), nq, k)
                assert r[2]["scan_rows"] == code, (what, leg, r[2]["scan_rows"])
                assert r[2]["brute_rows"] > 0, (what, leg)  # (a batch that scans nothing shows nothing)
        finally:
            self.leg("off")
            if exact:
                self.idx.set_exact_windows(0)
        for leg in ("half", "byte"):
            assert np.array_equal(rows[leg][0], rows["off"][0]), ("ids", what, leg)
            assert np.array_equal(rows[leg][1], rows["off"][1]), ("distance bits", what, leg)
            for key in WORK:
                assert rows[leg][2][key] == rows["off"][2][key], (key, what, leg, rows[leg][2][key], rows["off"][2][key])
        return rows["off"]


@pytest.fixture(scope="module")
def built(wa, gpu, tmp_path_factory):
    torch = pytest.importorskip("torch")
    made = {}

    def get(name):
        if name not in made:
            cls, data, kw = CASES[name]
            X, Q = data()
            # (a graph cache of its own: the oracle loads the graphs this index was built with)
            made[name] = Built(wa, torch, cls, X, Q, kw, str(tmp_path_factory.mktemp(name)) + "/")
            idx = made[name].idx
            # a new index: both copies, the switch off
            assert idx.scan_rows() is False and idx.half_rows() is True and idx.byte_rows() is False
            assert idx.half_rows_bytes() > 0 and idx.byte_rows_bytes() > 0
        return made[name]

    return get


def _oracle_index(oracle, b):
    return getattr(oracle, b.cls)(b.X, b.labels, build_params=oracle.BuildParams(32, 64, 1.0, b.cache), **b.kw)


def _against(oracle_rows, got, ctx, what):
    eids, edists = oracle_rows
    ok, why = gu.same_rows(eids.view(np.uint32), edists, got[0], got[1].view(np.float32), True, ctx)
    assert ok, (what, why)


@pytest.mark.parametrize("name", ["sift128_l2_tree", "sift20_l2_tree", "sift200_l2_tree", "ties6_l2_tree"])
def test_tiny_windows_and_whole_scans_of_a_tree(built, wa, oracle, name):
    """optimized_postfilter with windows below the tiny-window rule (47 points: 4 w < cutoff, every query is a scan) at k = 1, 10
    and 100 -- more than the window holds: the padding -- and 24 wider windows (1 509 points: 23 full passes and a tail) scanned
    because of set_exact_windows.  The k = 10 tiny-window rows against the CPU oracle."""
    b = built(name)
    W = windows(b.labels, NQ, -7, 71)
    off = {}
    for k in (1, 10, 100):
        for form in ("host", "device"):
            off[k, form] = b.three_ways(wa, W, k=k, form=form, what=(name, "tiny", k, form))
            assert off[k, form][2]["beam_searches"] == 0
        assert np.array_equal(off[k, "host"][0], off[k, "device"][0]) and np.array_equal(off[k, "host"][1], off[k, "device"][1])
    W2 = windows(b.labels, 24, -2, 72)
    for k in (10, 100):
        r = b.three_ways(wa, W2, k=k, exact=N, what=(name, "exact windows", k))
        assert r[2]["brute_rows"] == 24 * int(N * 0.25) and r[2]["beam_searches"] == 0
    oi = _oracle_index(oracle, b)
    exp = oi.batch_search(b.Q, W, NQ, "optimized_postfilter", _qp(oracle))
    _against(exp, off[10, "host"], gu.RowContext(b.X, b.labels, b.Q, W, "l2", "half_open"), name)


def test_inner_product_scans_of_a_super_tree(built, wa, oracle):
    """d = 100 under the inner product, set_exact_windows(n): batches of 24 queries (below the dense path's 32) are scanned --
    windows of an eighth and of half of the points; against the oracle's PrefilterIndex on the same points"""
    b = built("sift100_mips_super")
    for p, k in ((-3, 10), (-1, 10), (-3, 1), (-1, 100)):
        W = windows(b.labels, 24, p, 73)
        r = b.three_ways(wa, W, k=k, exact=N, what=("mips super", p, k))
        assert r[2]["beam_searches"] == 0 and r[2]["brute_rows"] == 24 * int(N * 2.0 ** p)
        if k == 10:
            pi = oracle.PrefilterIndexFloatMips(b.X, b.labels)
            exp = pi.batch_search(b.Q[:24], W, 24, _qp(oracle))
            _against(exp, r, gu.RowContext(b.X, b.labels, b.Q[:24], W, "mips", "prefilter"), ("mips super", p))


@pytest.mark.parametrize("name", ["sift128_l2_tree", "sift20_l2_tree"])
def test_windows_of_exact_widths(built, wa, oracle, name):
    """windows of exactly 1, 63, 64, 65, 127 and 129 points placed by label rank -- at the start of the set, in the middle at an
    odd first row, ending on the last row -- each one a scan because of set_exact_windows; k = 1, 10 (more than the narrowest
    window holds) and 100.  The oracle's tree scans such windows too (4 w < cutoff): its rows at k = 10."""
    b = built(name)
    a = [0] * 6 + [3001] * 6 + [N - w for w in WIDTHS]
    e = [w for w in WIDTHS] + [3001 + w for w in WIDTHS] + [N] * 6
    W = b.rank_windows(a, e)
    got = {}
    for k in (1, 10, 100):
        got[k] = r = b.three_ways(wa, W, k=k, exact=200, what=(name, "widths", k))
        assert r[2]["brute_rows"] == 3 * sum(WIDTHS) and r[2]["beam_searches"] == 0
        found = (r[1].view(np.float32) != np.finfo(np.float32).max).sum(axis=1)
        assert found.tolist() == [min(w, k) for w in WIDTHS] * 3, (name, k)
    oi = _oracle_index(oracle, b)
    exp = oi.batch_search(b.Q[:18], W, 18, "optimized_postfilter", _qp(oracle))
    _against(exp, got[10], gu.RowContext(b.X, b.labels, b.Q[:18], W, "l2", "half_open"), name)


@pytest.mark.parametrize("method", ["fenwick", "three_split"])
def test_end_scans_of_the_multi_bucket_methods(built, wa, oracle, method):
    """half of the points per window (3 018, three leaves' worth): a cover of buckets that are searched and two ends that are scanned"""
    b = built("sift128_l2_tree")
    W = windows(b.labels, NQ, -1, 74)
    r = b.three_ways(wa, W, method=method, beam=40, what=method)
    assert r[2]["beam_searches"] > 0 and r[2]["brute_rows"] > NQ
    r2 = b.three_ways(wa, W, method=method, beam=40, form="device", what=(method, "device"))
    assert np.array_equal(r[0], r2[0]) and np.array_equal(r[1], r2[1])
    oi = _oracle_index(oracle, b)
    exp = oi.batch_search(b.Q, W, NQ, method, _qp(oracle, 10, 40))
    _against(exp, r, gu.RowContext(b.X, b.labels, b.Q, W, "l2", gu.window_rule("VamanaRangeFilterTreeIndex", method)), method)


@pytest.mark.parametrize("name", ["sift128_l2_tree", "sift100_mips_super"])
def test_the_sliced_scan(built, wa, name):
    """two queries whose windows are the whole set: k_brute cuts each scan into slices, one wave each, and the last slice merges"""
    b = built(name)
    W = np.array([[b.sorted[0] - 1, b.sorted[-1] + 1]] * 2, dtype=np.float64)
    for k in (10, 100):
        r = b.three_ways(wa, W, k=k, exact=N, what=(name, "sliced", k))
        assert r[2]["brute_rows"] == 2 * N and r[2]["beam_searches"] == 0


def test_an_asynchronous_pair_keeps_what_it_was_submitted_with(built, wa):
    """two batches on the asynchronous lanes, the switch changed between the two submissions: each ticket reports its own"""
    b = built("sift128_l2_tree")
    idx, torch = b.idx, b.torch
    W = windows(b.labels, NQ, -7, 71).astype(np.float32)
    want = b.three_ways(wa, W, what="async reference")
    tw = torch.from_numpy(W).to(b.dev)
    out = [(torch.zeros((NQ, 10), dtype=torch.int32, device=b.dev), torch.zeros((NQ, 10), dtype=torch.float32, device=b.dev)) for _ in range(2)]
    torch.cuda.synchronize()
    try:
        for first, second in ((("byte", 2), ("off", 0)), (("off", 0), ("half", 1))):
            tickets = []
            for (leg, _), (ti, td) in zip((first, second), out):
                b.leg(leg)
                tickets.append(idx.batch_search_device_async(b.tq.data_ptr(), tw.data_ptr(), NQ, 0, "optimized_postfilter", _qp(wa), ti.data_ptr(), td.data_ptr(), 0))
            b.leg("off" if second[0] != "off" else "byte")  # (and once more before either is waited for)
            for t, (leg, code), (ti, td) in zip(tickets, (first, second), out):
                c = idx.wait(t)
                assert c["scan_rows"] == code, (leg, c["scan_rows"])
                assert np.array_equal(ti.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(td.cpu().numpy().view(np.uint32), want[1]), leg
                for key in WORK:
                    assert c[key] == want[2][key], (key, leg)
    finally:
        b.leg("off")


def test_indexes_without_a_copy_and_with_half_rows_only(built, wa):
    """no shadow copy at all: the switch stays off and rows and counters are those of before.  Half rows but no one-byte rows
    (one value 256.0, or one value 0.5 -- both binary16 values): the switch on reads the half rows, never the one-byte rows."""
    torch = pytest.importorskip("torch")
    X, Q = _sift(128, 61)
    labels = distinct_labels(N, 9)
    W = windows(labels, NQ, -7, 71)
    kw = dict(cutoff=1000, split_factor=2)

    def refuses(idx, search):
        before = search()
        c0 = idx.counters()
        assert idx.scan_rows() is False and idx.set_scan_rows(True) is False and idx.scan_rows() is False
        after = search()
        c1 = idx.counters()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        assert c1["scan_rows"] == 0 and c1["brute_rows"] > 0
        for key in WORK:
            assert c0[key] == c1[key], key

    pre = wa.PrefilterIndexFloatEuclidian(X, labels)
    refuses(pre, lambda: pre.batch_search(Q, W, NQ, _qp(wa)))
    Xb = X.copy()
    Xb[N // 3, 7] = np.float32(1.0) / np.float32(3.0)  # (no binary16 value: neither copy)
    bad = getattr(wa, TREE)(Xb, labels, build_params=wa.BuildParams(32, 64, 1.0, ""), **kw)
    assert bad.half_rows_bytes() == 0 and bad.byte_rows_bytes() == 0
    refuses(bad, lambda: bad.batch_search(Q, W, NQ, "optimized_postfilter", _qp(wa)))
    u8 = wa.VamanaRangeFilterTreeIndexUInt8Euclidian(X.astype(np.uint8), labels, build_params=wa.BuildParams(32, 64, 1.0, ""), **kw)
    Q8 = np.rint(Q).astype(np.uint8)
    refuses(u8, lambda: u8.batch_search(Q8, W, NQ, "optimized_postfilter", _qp(wa)))
    want = built("sift128_l2_tree").three_ways(wa, W, what="reference")
    for value in (256.0, 0.5):
        Xh = X.copy()
        Xh[N // 3, 7] = value
        half = Built(wa, torch, TREE, Xh, Q, kw)
        idx = half.idx
        assert idx.half_rows_bytes() > 0 and idx.byte_rows_bytes() == 0
        off = half.call("host", W, "optimized_postfilter", _qp(wa), NQ, 10)
        assert off[2]["scan_rows"] == 0 and off[2]["brute_rows"] > 0
        assert idx.set_scan_rows(True) is True and idx.set_byte_rows(True) is False
        on = half.call("host", W, "optimized_postfilter", _qp(wa), NQ, 10)
        assert on[2]["scan_rows"] == 1 and on[2]["byte_rows"] == 0, value
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
        for key in WORK:
            assert on[2][key] == off[2][key] == want[2][key], key
        assert idx.set_half_rows(False) is False  # (the switch stays on, and the scan goes back to the index's own rows)
        own = half.call("host", W, "optimized_postfilter", _qp(wa), NQ, 10)
        assert idx.scan_rows() is True and own[2]["scan_rows"] == 0
        assert np.array_equal(own[0], off[0]) and np.array_equal(own[1], off[1])
