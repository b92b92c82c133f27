"""GPU: the half-precision shadow rows of a float32 index (include/wann.h, wann_set_half_rows).  A float32 index with graphs
whose points are all finite binary16 values keeps a second copy of its rows as halves, and its beam searches read that copy
through the float16 unit's kernels.  Those score a row in the float32 kernels' arithmetic and order after an exact conversion,
so ids, distance bits and the operation counters must not depend on the switch, in any core, method or call form."""
import numpy as np
import pytest

import golden_util as gu
from util import distinct_labels, sift_like, unit_mixture, windows

pytestmark = pytest.mark.gpu
N, NQ, K = 30000, 600, 10
WORK = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads")


def _qp(mod, beam, mult=1):
    return mod.QueryParams(K, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)


def _sift(d, seed):
    g = sift_like(N, d, seed)
    return g(N), g(NQ)


def _mixture16(d, seed):
    g = unit_mixture(N, d, seed)
    return g(N).astype(np.float16).astype(np.float32), g(NQ)  # (points rounded through float16; queries are NOT)


CASES = {
    "sift128_l2_tree": ("VamanaRangeFilterTreeIndexFloatEuclidian", lambda: _sift(128, 41), dict(cutoff=500, split_factor=2)),
    "mixture100_mips_super": ("SuperOptimizedPostfilterTreeIndexFloatMips", lambda: _mixture16(100, 42),
                              dict(cutoff=400, split_factor=2, shift_factor=0.5)),
    "sift20_l2_tree": ("VamanaRangeFilterTreeIndexFloatEuclidian", lambda: _sift(20, 43), dict(cutoff=500, split_factor=2)),
}


class Built:
    def __init__(self, wa, torch, cls, X, Q, kw, cache=""):
        self.labels = distinct_labels(N, 9)
        self.X, self.Q = X, Q
        self.idx = getattr(wa, cls)(X, self.labels, build_params=wa.BuildParams(32, 64, 1.0, cache), **kw)
        self.tree = cls.startswith("VamanaRangeFilterTreeIndex")
        self.dev = torch.device("cuda:0")
        self.tq = torch.from_numpy(Q).to(self.dev)
        self.qids = torch.arange(NQ, dtype=torch.int64, device=self.dev)
        self.ti = torch.empty((NQ, K), dtype=torch.int32, device=self.dev)
        self.td = torch.empty((NQ, K), dtype=torch.float32, device=self.dev)
        self.torch = torch

    def _out(self):
        return self.ti.cpu().numpy().view(np.uint32).copy(), self.td.cpu().numpy().view(np.uint32).copy()

    def call(self, form, W, method, qp):
        """rows (ids, distance bits) and counters of one batch through one of the four call forms"""
        idx, torch = self.idx, self.torch
        if form == "host":
            a = (method,) if self.tree else ()
            ids, dists = idx.batch_search(self.Q, W, NQ, *a, qp)
            return ids.copy(), dists.view(np.uint32).copy(), idx.counters()
        tw = torch.from_numpy(W).to(self.dev)
        self.ti.zero_()
        self.td.zero_()
        torch.cuda.synchronize()
        m = method if self.tree else ""
        p = (self.ti.data_ptr(), self.td.data_ptr(), 0)
        if form == "device":
            idx.batch_search_device(self.tq.data_ptr(), tw.data_ptr(), NQ, 0, m, qp, *p)
            c = idx.counters()
        elif form == "async":
            c = idx.wait(idx.batch_search_device_async(self.tq.data_ptr(), tw.data_ptr(), NQ, 0, m, qp, *p))
        else:
            idx.batch_search_device_ids(self.tq.data_ptr(), tw.data_ptr(), NQ, self.qids.data_ptr(), m, qp, *p)
            c = idx.counters()
        return self._out() + (c,)


@pytest.fixture(scope="module")
def built(wa, gpu):
    torch = pytest.importorskip("torch")
    cache = {}

    def get(name):
        if name not in cache:
            cls, data, kw = CASES[name]
            X, Q = data()
            cache[name] = Built(wa, torch, cls, X, Q, kw)
        return cache[name]

    return get


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), ("ids", what)
    assert np.array_equal(a[1], b[1]), ("distance bits", what)
    for key in WORK:
        assert a[2][key] == b[2][key], (key, what, a[2][key], b[2][key])


@pytest.mark.parametrize("name", list(CASES))
def test_rows_do_not_depend_on_the_row_store(built, wa, name):
    """both register cores (beams 10 and 40 x 2 = 80), the LDS-beam core (200) and the doubling loop (narrow windows), through
    the host, device, asynchronous and per-query-id calls"""
    b = built(name)
    idx = b.idx
    assert idx.half_rows() is True and idx.half_rows_bytes() > 0
    for p in (-9, -5, -3, 0):
        W = windows(b.labels, NQ, p, 70 + p).astype(np.float32)
        for beam, mult in ((10, 1), (40, 2), (200, 1)):
            qp = _qp(wa, beam, mult)
            rows = {}
            for on in (False, True):
                assert idx.set_half_rows(on) is on
                for form in ("host", "device", "async", "ids"):
                    r = b.call(form, W, "optimized_postfilter", qp)
                    assert r[2]["half_rows"] == (1 if on else 0), (form, on)
                    # (2^-9 of 30 000 points is 58 points: below the cutoff such a window is scanned, on the float32 rows)
                    assert r[2]["beam_searches"] > 0 or p == -9
                    rows[on, form] = r
            for form in ("host", "device", "async", "ids"):
                _same(rows[True, form], rows[False, form], (name, p, beam, mult, form))
                _same(rows[True, form], rows[False, "host"], (name, p, beam, mult, form, "vs host"))
    assert idx.set_half_rows(True) is True


@pytest.mark.parametrize("method", ["three_split", "fenwick"])
def test_multi_bucket_methods(built, wa, method):
    """their end scans stay on the float32 rows (k_brute), their graph searches read the shadow"""
    b = built("sift128_l2_tree")
    W = windows(b.labels, NQ, -5, 65).astype(np.float32)
    qp = _qp(wa, 40, 2)
    rows = {}
    for on in (False, True):
        assert b.idx.set_half_rows(on) is on
        for form in ("host", "device"):
            rows[on, form] = b.call(form, W, method, qp)
            assert rows[on, form][2]["half_rows"] == (1 if on else 0)
    for form in ("host", "device"):
        _same(rows[True, form], rows[False, form], (method, form))
    assert rows[True, "host"][2]["brute_rows"] > 0 and rows[True, "host"][2]["beam_searches"] > 0


def test_alternation_with_batches_in_flight(built, wa):
    """off / on / off over three consecutive batches of one index, an asynchronous batch in flight at every toggle: the lanes'
    and the blocking call's workspaces are sized per batch by the view in use.  A batch keeps the setting it was submitted with."""
    b = built("sift128_l2_tree")
    idx, torch = b.idx, b.torch
    qp = _qp(wa, 40, 2)
    W = windows(b.labels, NQ, -3, 67).astype(np.float32)
    idx.set_half_rows(True)
    want = b.call("host", W, "optimized_postfilter", qp)
    tw = torch.from_numpy(W).to(b.dev)
    ai = torch.zeros((NQ, K), dtype=torch.int32, device=b.dev)
    ad = torch.zeros((NQ, K), dtype=torch.float32, device=b.dev)
    before = True
    for on in (False, True, False):
        ai.zero_()
        ad.zero_()
        torch.cuda.synchronize()
        t = idx.batch_search_device_async(b.tq.data_ptr(), tw.data_ptr(), NQ, 0, "optimized_postfilter", qp, ai.data_ptr(), ad.data_ptr(), 0)
        assert idx.set_half_rows(on) is on
        got = b.call("device", W, "optimized_postfilter", qp)
        assert got[2]["half_rows"] == (1 if on else 0)
        _same(got, want, ("blocking", on))
        c = idx.wait(t)
        assert c["half_rows"] == (1 if before else 0)
        _same((ai.cpu().numpy().view(np.uint32), ad.cpu().numpy().view(np.uint32), c), want, ("in flight", on))
        before = on
    idx.set_half_rows(True)


def test_ineligible_points_have_no_shadow(built, wa, oracle, tmp_path):
    """one value that is no binary16 value: no shadow, the switch stays off, and the index is the float32 index it always was --
    rows and operation counts of the oracle for one small batch.  Its device_bytes are those of the eligible index of the same
    shape, which therefore does not count its shadow."""
    torch = pytest.importorskip("torch")
    cls, data, kw = CASES["sift128_l2_tree"]
    X, Q = data()
    X = X.copy()
    X[N // 3, 7] = 0.1
    cache = str(tmp_path) + "/"
    bad = Built(wa, torch, cls, X, Q, kw, cache)
    idx = bad.idx
    assert idx.half_rows() is False and idx.half_rows_bytes() == 0
    assert idx.set_half_rows(True) is False and idx.half_rows() is False
    good = built("sift128_l2_tree").idx
    assert idx.device_bytes() == good.device_bytes()
    assert good.half_rows_bytes() == N * 64 * -(-2 * 128 // 64)
    assert built("sift20_l2_tree").idx.half_rows_bytes() == N * 64  # (40 bytes of halves in a 64-byte row)
    assert built("mixture100_mips_super").idx.half_rows_bytes() == N * 64 * 4
    was = good.device_bytes()
    good.set_half_rows(False)
    assert good.device_bytes() == was and good.half_rows_bytes() == N * 256  # (the switch allocates and frees nothing)
    good.set_half_rows(True)
    nq = 100
    oi = getattr(oracle, cls)(X, bad.labels, build_params=oracle.BuildParams(32, 64, 1.0, cache), **kw)
    for p in (-5, -3):
        W = windows(bad.labels, nq, p, 80 + p)
        for beam, mult in ((10, 1), (40, 2)):
            ids, dists = idx.batch_search(Q[:nq], W, nq, "optimized_postfilter", _qp(wa, beam, mult))
            c = idx.counters()
            eids, edists = oi.batch_search(Q[:nq], W, nq, "optimized_postfilter", _qp(oracle, beam, mult))
            ok, why = gu.same_rows(eids, edists, ids, dists, False, gu.RowContext(X, bad.labels, Q[:nq], W, gu.metric_of("Euclidian")))
            assert ok, (p, beam, mult, why)
            oc = oi.last_counters
            assert c["half_rows"] == 0
            assert c["beam_searches"] == oc["searches"] and c["hops"] == oc["hops"], (p, beam)
            assert c["dist_cmps"] + c["brute_rows"] == oc["dist_cmps"], (p, beam)
