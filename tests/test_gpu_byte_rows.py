"""GPU: the one-byte shadow rows of a float32 index (include/wann.h, wann_set_byte_rows).  A float32 index with graphs whose
points are all integers 0 .. 255 keeps a third copy of its rows as uint8, and -- once asked to -- its beam searches read that
copy through the kernels of wann_kernels_w8.hip.  Those widen every byte to the float32 it was made from and then run the
float32 kernels' arithmetic in its order against the caller's float32 query, so ids, distance bits and the operation counters
must not depend on the row store (float32 rows, half rows, one-byte rows), in any core, method or call form.

The queries are NOT integers (sift-like queries plus uniform noise): their fp32 sums depend on the evaluation order, so equal
distance bits show that the order was kept.  Values of 128 and above occur in every point set: a signed widening would show."""
import numpy as np
import pytest

import golden_util as gu
from util import distinct_labels, sift_like, windows

pytestmark = pytest.mark.gpu
N, NQ, K = 30000, 600, 10
WORK = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads")
STORES = ("f32", "half", "byte")
FORMS = ("host", "device", "async", "ids")


def _qp(mod, beam, mult=1):
    return mod.QueryParams(K, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)


def _sift(d, seed):
    g = sift_like(N, d, seed)
    X, Q = g(N), g(NQ)
    # numpy's clip keeps the -0.0 that rint makes of values in (-0.5, 0): a few thousand elements here.  The rule is on bits and
    # refuses -0.0 (tests/test_byte_rows_api.py), so the zeros are made +0.0: the same values, integers in [0, 255]
    assert np.signbit(X).any()
    X = X + np.float32(0)
    assert not np.signbit(X).any() and X.dtype == np.float32
    assert X.min() >= 0 and X.max() <= 255 and (X >= 128).any() and np.array_equal(X, np.rint(X))
    Q = (Q + np.random.default_rng(seed + 1000).random(Q.shape, dtype=np.float32)).astype(np.float32)
    assert not np.array_equal(Q, np.rint(Q))
    return X, Q


# d = 128: compile-time block count 16, the two-row routines, the 16-block register-resident mid core; d = 100: 13 blocks with a
# tail under the inner product, 100 bytes in a 128-byte row; d = 20: run-time odd block count 3, 44 padding bytes; d = 200: a
# 256-byte stride, more than one 128-byte line per row
CASES = {
    "sift128_l2_tree": ("VamanaRangeFilterTreeIndexFloatEuclidian", lambda: _sift(128, 51), dict(cutoff=500, split_factor=2)),
    "sift100_mips_super": ("SuperOptimizedPostfilterTreeIndexFloatMips", lambda: _sift(100, 52),
                           dict(cutoff=400, split_factor=2, shift_factor=0.5)),
    "sift20_l2_tree": ("VamanaRangeFilterTreeIndexFloatEuclidian", lambda: _sift(20, 53), dict(cutoff=500, split_factor=2)),
    "sift200_l2_tree": ("VamanaRangeFilterTreeIndexFloatEuclidian", lambda: _sift(200, 54), dict(cutoff=500, split_factor=2)),
}
DIMS = {"sift128_l2_tree": 128, "sift100_mips_super": 100, "sift20_l2_tree": 20, "sift200_l2_tree": 200}


class Built:
    def __init__(self, wa, torch, cls, X, Q, kw, cache=""):
        self.labels = distinct_labels(N, 9)
        self.cls, self.kw, self.cache = cls, kw, cache
        self.X, self.Q = X, Q
        self.idx = getattr(wa, cls)(X, self.labels, build_params=wa.BuildParams(32, 64, 1.0, cache), **kw)
        self.tree = cls.startswith("VamanaRangeFilterTreeIndex")
        self.dev = torch.device("cuda:0")
        self.tq = torch.from_numpy(Q).to(self.dev)
        self.qids = torch.arange(NQ, dtype=torch.int64, device=self.dev)
        self.ti = torch.empty((NQ, K), dtype=torch.int32, device=self.dev)
        self.td = torch.empty((NQ, K), dtype=torch.float32, device=self.dev)
        self.torch = torch
        # what a new index starts with: the setting, and the store its first batch reads
        W = windows(self.labels, NQ, -3, 67).astype(np.float32)
        self.first = (self.idx.byte_rows(), self.idx.half_rows(), self.call("host", W, "optimized_postfilter", _qp(wa, 40, 2))[2])

    def store(self, which):
        """the row store of the next batches; the one-byte rows go before the half rows, whose switch stays on under them"""
        idx = self.idx
        assert idx.set_byte_rows(which == "byte") is (which == "byte")
        assert idx.set_half_rows(which != "f32") is (which != "f32")
        assert idx.byte_rows() is (which == "byte") and idx.half_rows() is (which != "f32")

    def call(self, form, W, method, qp, nq=NQ):
        """rows (ids, distance bits) and counters of one batch of the first nq queries through one of the four call forms"""
        idx, torch = self.idx, self.torch
        if form == "host":
            a = (method,) if self.tree else ()
            ids, dists = idx.batch_search(self.Q[:nq], W, nq, *a, qp)
            return ids.copy(), dists.view(np.uint32).copy(), idx.counters()
        tw = torch.from_numpy(W).to(self.dev)
        self.ti.zero_()
        self.td.zero_()
        torch.cuda.synchronize()
        m = method if self.tree else ""
        p = (self.ti.data_ptr(), self.td.data_ptr(), 0)
        if form == "device":
            idx.batch_search_device(self.tq.data_ptr(), tw.data_ptr(), nq, 0, m, qp, *p)
            c = idx.counters()
        elif form == "async":
            c = idx.wait(idx.batch_search_device_async(self.tq.data_ptr(), tw.data_ptr(), nq, 0, m, qp, *p))
        else:
            idx.batch_search_device_ids(self.tq.data_ptr(), tw.data_ptr(), nq, self.qids.data_ptr(), m, qp, *p)
            c = idx.counters()
        return self.ti.cpu().numpy().view(np.uint32)[:nq].copy(), self.td.cpu().numpy().view(np.uint32)[:nq].copy(), c


@pytest.fixture(scope="module")
def built(wa, gpu, tmp_path_factory):
    torch = pytest.importorskip("torch")
    made = {}

    def get(name):
        if name not in made:
            cls, data, kw = CASES[name]
            X, Q = data()
            # (a graph cache of its own: the oracle of test_byte_rows_against_the_oracle loads the graphs this index was built with)
            made[name] = Built(wa, torch, cls, X, Q, kw, str(tmp_path_factory.mktemp(name)) + "/")
        return made[name]

    return get


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), ("ids", what)
    assert np.array_equal(a[1], b[1]), ("distance bits", what)
    for key in WORK:
        assert a[2][key] == b[2][key], (key, what, a[2][key], b[2][key])


def _reports(c, store, what):
    assert c["byte_rows"] == (1 if store == "byte" else 0), (what, c["byte_rows"])
    assert c["half_rows"] == (1 if store == "half" else 0), (what, c["half_rows"])


@pytest.mark.parametrize("name", list(CASES))
def test_rows_do_not_depend_on_the_row_store(built, wa, name):
    """both register cores (beams 10 and 40 x 2 = 80), the LDS-beam cores (200, 400), the doubling loop (narrow windows) and, on
    d = 128, the one-wave core (beam 2000), through the host, device, asynchronous and per-query-id calls"""
    b = built(name)
    idx = b.idx
    assert idx.byte_rows() is False and idx.byte_rows_bytes() > 0 and idx.half_rows() is True
    try:
        for p in (-9, -5, -3, 0):
            W = windows(b.labels, NQ, p, 70 + p).astype(np.float32)
            for beam, mult in ((10, 1), (40, 2), (200, 1), (400, 1)):
                qp = _qp(wa, beam, mult)
                rows = {}
                for store in STORES:
                    b.store(store)
                    for form in FORMS:
                        r = b.call(form, W, "optimized_postfilter", qp)
                        _reports(r[2], store, (name, p, beam, store, form))
                        # (2^-9 of 30 000 points is 58 points: below the cutoff such a window is scanned, on the float32 rows)
                        assert r[2]["beam_searches"] > 0 or p == -9
                        rows[store, form] = r
                for form in FORMS:
                    for store in ("half", "byte"):
                        _same(rows[store, form], rows["f32", form], (name, p, beam, mult, store, form))
                    _same(rows["byte", form], rows["f32", "host"], (name, p, beam, mult, form, "vs host"))
        if name == "sift128_l2_tree":
            nq = 50
            W = windows(b.labels, nq, 0, 71).astype(np.float32)
            rows = {}
            for store in STORES:
                b.store(store)
                rows[store] = b.call("host", W, "optimized_postfilter", _qp(wa, 2000), nq)
                _reports(rows[store][2], store, (name, "beam 2000", store))
                assert rows[store][2]["beam_searches"] >= nq
            _same(rows["half"], rows["f32"], (name, "beam 2000", "half"))
            _same(rows["byte"], rows["f32"], (name, "beam 2000", "byte"))
        # the one-byte rows go first whatever the half rows' switch says
        assert idx.set_half_rows(False) is False and idx.set_byte_rows(True) is True
        W = windows(b.labels, NQ, -3, 67).astype(np.float32)
        _reports(b.call("device", W, "optimized_postfilter", _qp(wa, 40, 2))[2], "byte", (name, "half rows off"))
    finally:
        b.store("half")  # (what a new index starts with)


@pytest.mark.parametrize("method", ["three_split", "fenwick"])
def test_multi_bucket_methods(built, wa, method):
    """their end scans stay on the float32 rows (k_brute), their graph searches read the one-byte rows"""
    b = built("sift128_l2_tree")
    W = windows(b.labels, NQ, -5, 65).astype(np.float32)
    qp = _qp(wa, 40, 2)
    rows = {}
    try:
        for store in STORES:
            b.store(store)
            for form in ("host", "device"):
                rows[store, form] = b.call(form, W, method, qp)
                _reports(rows[store, form][2], store, (method, store, form))
    finally:
        b.store("half")
    for form in ("host", "device"):
        _same(rows["half", form], rows["f32", form], (method, form, "half"))
        _same(rows["byte", form], rows["f32", form], (method, form, "byte"))
    assert rows["byte", "host"][2]["brute_rows"] > 0 and rows["byte", "host"][2]["beam_searches"] > 0


def test_alternation_with_batches_in_flight(built, wa):
    """off / byte / half / byte over four consecutive batches of one index, an asynchronous batch in flight at every toggle: the
    lanes' and the blocking call's workspaces are sized per batch by the view in use.  A batch keeps the store it was submitted with."""
    b = built("sift128_l2_tree")
    idx, torch = b.idx, b.torch
    qp = _qp(wa, 40, 2)
    W = windows(b.labels, NQ, -3, 67).astype(np.float32)
    b.store("half")
    want = b.call("host", W, "optimized_postfilter", qp)
    tw = torch.from_numpy(W).to(b.dev)
    ai = torch.zeros((NQ, K), dtype=torch.int32, device=b.dev)
    ad = torch.zeros((NQ, K), dtype=torch.float32, device=b.dev)
    before = "half"
    try:
        for store in ("f32", "byte", "half", "byte"):
            ai.zero_()
            ad.zero_()
            torch.cuda.synchronize()
            t = idx.batch_search_device_async(b.tq.data_ptr(), tw.data_ptr(), NQ, 0, "optimized_postfilter", qp, ai.data_ptr(), ad.data_ptr(), 0)
            b.store(store)
            got = b.call("device", W, "optimized_postfilter", qp)
            _reports(got[2], store, ("blocking", store))
            _same(got, want, ("blocking", store))
            c = idx.wait(t)
            _reports(c, before, ("in flight", before, store))
            _same((ai.cpu().numpy().view(np.uint32), ad.cpu().numpy().view(np.uint32), c), want, ("in flight", store))
            before = store
    finally:
        b.store("half")


@pytest.mark.parametrize("name", list(CASES))
def test_byte_rows_against_the_oracle(built, wa, oracle, name):
    """one small batch per shape with the one-byte rows on, against the CPU restatement: the rows of the new unit rest on the
    reference's arithmetic, not only on the sibling kernels"""
    b = built(name)
    nq = 100
    oi = getattr(oracle, b.cls)(b.X, b.labels, build_params=oracle.BuildParams(32, 64, 1.0, b.cache), **b.kw)
    W = windows(b.labels, nq, -3, 77)
    m = ("optimized_postfilter",) if b.tree else ()
    try:
        b.store("byte")
        ids, dists = b.idx.batch_search(b.Q[:nq], W, nq, *m, _qp(wa, 40, 2))
        c = b.idx.counters()
    finally:
        b.store("half")
    eids, edists = oi.batch_search(b.Q[:nq], W, nq, *m, _qp(oracle, 40, 2))
    ok, why = gu.same_rows(eids, edists, ids, dists, False, gu.RowContext(b.X, b.labels, b.Q[:nq], W, gu.metric_of(b.cls)))
    assert ok, (name, why)
    oc = oi.last_counters
    assert c["byte_rows"] == 1 and c["half_rows"] == 0
    assert c["beam_searches"] == oc["searches"] and c["hops"] == oc["hops"], name
    assert c["dist_cmps"] + c["brute_rows"] == oc["dist_cmps"], name


def test_ineligible_sets_and_bookkeeping(built, wa):
    """one value that is no uint8 value: no one-byte copy, the switch stays off; what the copy costs; what device_bytes counts;
    what a new index starts with"""
    torch = pytest.importorskip("torch")
    cls, data, kw = CASES["sift128_l2_tree"]
    X, Q = data()
    good = built("sift128_l2_tree").idx
    for bad_value, half in ((0.5, True), (256.0, True)):  # (both are binary16 values: the half rows stay)
        Xb = X.copy()
        Xb[N // 3, 7] = bad_value
        bad = Built(wa, torch, cls, Xb, Q, kw)
        idx = bad.idx
        assert idx.byte_rows() is False and idx.byte_rows_bytes() == 0
        assert idx.set_byte_rows(True) is False and idx.byte_rows() is False
        assert idx.half_rows() is half and idx.half_rows_bytes() == good.half_rows_bytes()
        assert idx.device_bytes() == good.device_bytes()  # (which therefore counts neither copy)
        c = bad.first[2]  # (its first batch: the half rows, as ever)
        assert c["half_rows"] == 1 and c["byte_rows"] == 0 and c["beam_searches"] > 0
        del bad, idx
    for name, d in DIMS.items():
        assert built(name).idx.byte_rows_bytes() == N * 64 * -(-d // 64), name
    was = good.device_bytes()
    assert good.set_byte_rows(True) is True
    assert good.device_bytes() == was and good.byte_rows_bytes() == N * 128 and good.half_rows_bytes() == N * 256
    assert good.set_byte_rows(False) is False
    assert good.device_bytes() == was and good.byte_rows_bytes() == N * 128  # (the switch allocates and frees nothing)
    # an index without graphs has no copy and refuses the switch the same way
    pre = wa.PrefilterIndexFloatEuclidian(X[:4000], distinct_labels(4000, 9))
    assert pre.byte_rows() is False and pre.byte_rows_bytes() == 0 and pre.set_byte_rows(True) is False and pre.byte_rows() is False
    # a new index: the one-byte rows exist and are off, the first batch reads the half rows
    for name in CASES:
        byte_on, half_on, c = built(name).first
        assert byte_on is False and half_on is True, name
        assert c["half_rows"] == 1 and c["byte_rows"] == 0 and c["beam_searches"] > 0, name
