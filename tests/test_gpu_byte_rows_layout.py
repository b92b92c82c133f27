"""GPU: the interleaved layout of the one-byte shadow rows (include/wann.h wann_byte_row_position; wann_device.h u8_row_position).
The device copy permutes the bytes of every aligned group of 32 elements so that a lane of the kernels of wann_kernels_w8.hip
fetches four of its 4-element blocks with one 16-byte load (a quad); the blocks are still consumed in the float32 kernels'
order.  A wrong permutation, a wrong component of a quad or a changed order of the sums shows in the distance bits: the queries
are NOT integers, so their fp32 sums depend on the evaluation order, and every byte of a row enters its distance.  Every batch
therefore runs on the three row stores (float32 rows, half rows, one-byte rows) and ids, distance BITS and the work counters
must be equal -- no tolerance anywhere.

Row lengths tests/test_gpu_byte_rows.py does not reach, chosen for the quad fetch (a block = 8 elements of a lane pair):
  d =   8  one block: a quad that is mostly padding                      d =  96  compile-time 12, the two-row routines
  d =  40  five blocks, odd at run time, the last alone in quad 1        d = 100  compile-time 13, last block first (squared L2)
  d =  64  compile-time 8                                                d = 136  17 blocks, odd at run time, a 192-byte pitch
  d =  72  nine blocks, odd at run time                                  d = 264  33 blocks, a 320-byte pitch"""
import numpy as np
import pytest

import golden_util as gu
from util import distinct_labels, sift_like, windows

pytestmark = pytest.mark.gpu
N, NQ, K = 12000, 300, 10
WORK = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads")
STORES = ("f32", "half", "byte")
FORMS = ("host", "device")
L2, MIPS = "VamanaRangeFilterTreeIndexFloatEuclidian", "VamanaRangeFilterTreeIndexFloatMips"
KW = dict(cutoff=500, split_factor=2)
# (d, class): squared L2 at every length, the inner product where the issue asks for both
CASES = {f"d{d}_{'mips' if cls is MIPS else 'l2'}": (d, cls)
         for d, classes in ((8, (L2,)), (40, (L2, MIPS)), (64, (L2, MIPS)), (72, (L2,)), (96, (L2, MIPS)), (100, (L2,)),
                            (136, (L2, MIPS)), (264, (L2,)))
         for cls in classes}
SCAN_CASES = ("d40_l2", "d40_mips", "d100_l2", "d136_l2", "d136_mips")
ORACLE_CASES = ("d40_l2", "d40_mips", "d136_l2", "d136_mips")


def _qp(mod, beam, mult=1):
    return mod.QueryParams(K, beam, 1.35, 10_000_000, 10_000, mult, 10000, None, False)


def _sift(d, seed):
    g = sift_like(N, d, seed)
    X, Q = g(N) + np.float32(0), g(NQ)  # (+ 0: numpy's clip keeps the -0.0 that rint makes, and the one-byte rule is on bits)
    assert not np.signbit(X).any() and X.dtype == np.float32
    assert X.min() >= 0 and X.max() <= 255 and (X >= 128).any() and np.array_equal(X, np.rint(X))
    Q = (Q + np.random.default_rng(seed + 1000).random(Q.shape, dtype=np.float32)).astype(np.float32)
    assert not np.array_equal(Q, np.rint(Q))
    return X, Q


class Built:
    def __init__(self, wa, torch, cls, X, Q, cache):
        self.labels = distinct_labels(N, 9)
        self.cls, self.cache, self.X, self.Q = cls, cache, X, Q
        self.idx = getattr(wa, cls)(X, self.labels, build_params=wa.BuildParams(32, 64, 1.0, cache), **KW)
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.tq = torch.from_numpy(Q).to(self.dev)
        self.ti = torch.empty((NQ, K), dtype=torch.int32, device=self.dev)
        self.td = torch.empty((NQ, K), dtype=torch.float32, device=self.dev)

    def store(self, which):
        """the row store of the next batches; the one-byte rows go before the half rows, whose switch stays on under them"""
        idx = self.idx
        assert idx.set_byte_rows(which == "byte") is (which == "byte")
        assert idx.set_half_rows(which != "f32") is (which != "f32")

    def call(self, form, W, qp, nq=NQ):
        """rows (ids, distance bits) and counters of one batch of the first nq queries"""
        idx, torch = self.idx, self.torch
        if form == "host":
            ids, dists = idx.batch_search(self.Q[:nq], W, nq, "optimized_postfilter", qp)
            return ids.view(np.uint32).copy(), dists.view(np.uint32).copy(), idx.counters()
        tw = torch.from_numpy(np.asarray(W, dtype=np.float32)).to(self.dev)
        self.ti.zero_()
        self.td.zero_()
        torch.cuda.synchronize()
        idx.batch_search_device(self.tq.data_ptr(), tw.data_ptr(), nq, 0, "optimized_postfilter", qp, self.ti.data_ptr(), self.td.data_ptr(), 0)
        c = idx.counters()
        return self.ti.cpu().numpy().view(np.uint32)[:nq].copy(), self.td.cpu().numpy().view(np.uint32)[:nq].copy(), c


@pytest.fixture(scope="module")
def built(wa, gpu, tmp_path_factory):
    torch = pytest.importorskip("torch")
    made = {}

    def get(name):
        if name not in made:
            d, cls = CASES[name]
            X, Q = _sift(d, 300 + d)
            # (a graph cache of its own: the oracle loads the graphs this index was built with)
            made[name] = b = Built(wa, torch, cls, X, Q, str(tmp_path_factory.mktemp(name)) + "/")
            # a new index: both copies, the one-byte rows off, a pitch of 64-byte multiples whatever the layout inside it
            assert b.idx.byte_rows() is False and b.idx.half_rows() is True
            assert b.idx.byte_rows_bytes() == N * 64 * -(-d // 64), name
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
    """both register cores (beams 10 and 40 x 2 = 80) and the LDS-beam cores (200, 400) under windows of 2^-5, 2^-3 and all of
    the points, and on d = 96 the one-wave core (beam 2000 on 50 queries); host and device call forms"""
    b = built(name)
    try:
        for p in (-5, -3, 0):
            W = windows(b.labels, NQ, p, 80 + p).astype(np.float32)
            for beam, mult in ((10, 1), (40, 2), (200, 1), (400, 1)):
                qp = _qp(wa, beam, mult)
                rows = {}
                for store in STORES:
                    b.store(store)
                    for form in FORMS:
                        rows[store, form] = r = b.call(form, W, qp)
                        _reports(r[2], store, (name, p, beam, store, form))
                        assert r[2]["beam_searches"] > 0
                for form in FORMS:
                    for store in ("half", "byte"):
                        _same(rows[store, form], rows["f32", form], (name, p, beam, mult, store, form))
                    _same(rows["byte", form], rows["f32", "host"], (name, p, beam, mult, form, "vs host"))
        if CASES[name][0] == 96:
            nq = 50
            W = windows(b.labels, nq, 0, 81).astype(np.float32)
            rows = {}
            for store in STORES:
                b.store(store)
                rows[store] = b.call("host", W, _qp(wa, 2000), nq)
                _reports(rows[store][2], store, (name, "beam 2000", store))
                assert rows[store][2]["beam_searches"] >= nq
            _same(rows["half"], rows["f32"], (name, "beam 2000", "half"))
            _same(rows["byte"], rows["f32"], (name, "beam 2000", "byte"))
    finally:
        b.store("half")  # (what a new index starts with)


@pytest.mark.parametrize("name", SCAN_CASES)
def test_exact_scans_of_the_staged_rows(built, wa, name):
    """windows of 2^-9 of the points (23: below the tiny-window rule, every query is an exact scan) with set_scan_rows on and the
    one-byte rows selected -- k_brute_staged copies whole interleaved rows into the LDS, where a row starts on a multiple of 8,
    and scores them through the same routines -- against the switch off"""
    b = built(name)
    idx = b.idx
    W = windows(b.labels, NQ, -9, 82).astype(np.float32)
    qp = _qp(wa, 20)
    rows = {}
    try:
        for form in FORMS:
            b.store("half")
            assert idx.set_scan_rows(False) is False
            rows["off", form] = off = b.call(form, W, qp)
            assert off[2]["scan_rows"] == 0 and off[2]["brute_rows"] > 0 and off[2]["beam_searches"] == 0, (name, form)
            b.store("byte")
            assert idx.set_scan_rows(True) is True
            rows["on", form] = on = b.call(form, W, qp)
            assert on[2]["scan_rows"] == 2, (name, form, on[2]["scan_rows"])
            _same(on, off, (name, "staged scan", form))
        _same(rows["on", "device"], rows["off", "host"], (name, "staged scan", "device vs host"))
    finally:
        idx.set_scan_rows(False)
        b.store("half")


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_interleaved_rows_against_the_oracle(built, wa, oracle, name):
    """one batch of 100 queries with the one-byte rows on, against the CPU restatement: rows, searches and hops"""
    b = built(name)
    nq = 100
    oi = getattr(oracle, b.cls)(b.X, b.labels, build_params=oracle.BuildParams(32, 64, 1.0, b.cache), **KW)
    W = windows(b.labels, nq, -3, 83)
    try:
        b.store("byte")
        ids, dists = b.idx.batch_search(b.Q[:nq], W, nq, "optimized_postfilter", _qp(wa, 40, 2))
        c = b.idx.counters()
    finally:
        b.store("half")
    eids, edists = oi.batch_search(b.Q[:nq], W, nq, "optimized_postfilter", _qp(oracle, 40, 2))
    ok, why = gu.same_rows(eids, edists, ids, dists, False, gu.RowContext(b.X, b.labels, b.Q[:nq], W, gu.metric_of(b.cls)))
    assert ok, (name, why)
    oc = oi.last_counters
    assert c["byte_rows"] == 1 and c["half_rows"] == 0
    assert c["beam_searches"] == oc["searches"] and c["hops"] == oc["hops"], name
    assert c["dist_cmps"] + c["brute_rows"] == oc["dist_cmps"], name
