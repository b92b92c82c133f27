"""GPU: the paired layout of the half shadow rows (include/wann.h wann_half_row_position; wann_device.h h16_row_position).
The device copy permutes the halves of every aligned group of 16 elements so that a lane of the kernels of
wann_kernels_h16.hip fetches two of its 4-element blocks with one 16-byte load (a pair); the blocks are still consumed in the
float32 kernels' order.  A wrong permutation, a wrong half of a pair or a changed order of the sums shows in the distance
bits: the points are multiples of 1/8 in [-64, 192] (binary16 values, not integers, with -0.0 and magnitudes of 128 and more
among them), the queries are NOT binary16 values, so the fp32 sums depend on the evaluation order, and every half of a row
enters its distance.  Every batch runs with set_half_rows(True) and (False): ids, distance BITS and the work counters must be
equal -- no tolerance anywhere.

Row lengths chosen for the pair fetch (a block = 8 elements of a lane pair; sizes and helpers of tests/test_gpu_half_rows.py):
  d =   8   1 block:  a pair with one live block            d = 128  16: compile-time, the mid core; beam 2000: the one-wave core
  d =  20   3 blocks: odd at run time, block 2 alone        d = 136  17: above the held-row limit, odd, the batched run-time loop
  d =  40   5 blocks: odd, more than one pair               d = 200  25: a 448-byte pitch, four lines
  d = 100  13 blocks: the odd count held across the hop     d = 256  32: an even run-time count
            (under the inner product too: the fused tail)"""
import numpy as np
import pytest

import golden_util as gu
from test_gpu_half_rows import N, NQ, Built, _qp, _same
from util import windows

pytestmark = pytest.mark.gpu
L2, MIPS = "VamanaRangeFilterTreeIndexFloatEuclidian", "VamanaRangeFilterTreeIndexFloatMips"
KW = dict(cutoff=500, split_factor=2)
CASES = {f"d{d}_{'mips' if cls is MIPS else 'l2'}": (d, cls)
         for d, classes in ((8, (L2,)), (20, (L2,)), (40, (L2,)), (100, (L2, MIPS)), (128, (L2,)), (136, (L2,)), (200, (L2,)), (256, (L2,)))
         for cls in classes}
ORACLE_CASES = ("d136_l2", "d100_mips")
SCAN_CASES = ("d20_l2", "d100_mips", "d136_l2")
FORMS = ("host", "device", "async", "ids")


def _eighths(d, seed):
    """clustered rows (a few latent directions, as util.sift_like) on the grid of 1/8 in [-64, 192]; queries off every grid"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((16, d))

    def gen(m):
        x = rng.standard_normal((m, 16)) @ A * 18 + 64 + rng.standard_normal((m, d)) * 6
        return (np.clip(np.rint(x * 8), -512, 1536) / 8).astype(np.float32)

    X, Q = gen(N), gen(NQ)
    X[rng.random(X.shape) < 0.01] = np.float32(-0.0)
    assert np.array_equal(X, X.astype(np.float16).astype(np.float32)) and not np.array_equal(X, np.rint(X))
    assert X.min() >= -64 and X.max() <= 192 and (X >= 128).any() and (X < 0).any()
    assert (np.signbit(X) & (X == 0)).any()
    Q = (Q + rng.random(Q.shape, dtype=np.float32) / 8).astype(np.float32)
    assert not (Q == Q.astype(np.float16).astype(np.float32)).all(axis=1).any()
    return X, Q


@pytest.fixture(scope="module")
def built(wa, gpu, tmp_path_factory):
    torch = pytest.importorskip("torch")
    made = {}

    def get(name):
        if name not in made:
            d, cls = CASES[name]
            X, Q = _eighths(d, 500 + d)
            # (a graph cache of its own: the oracle loads the graphs this index was built with)
            cache = str(tmp_path_factory.mktemp(name)) + "/"
            made[name] = b = Built(wa, torch, cls, X, Q, KW, cache)
            b.cls, b.idx_cache = cls, cache
            # a new index: the half copy is on, the points hold -0.0 and fractions so there is no one-byte copy,
            # and the pitch is 64-byte multiples whatever the layout inside it
            assert b.idx.half_rows() is True and b.idx.byte_rows_bytes() == 0
            assert b.idx.half_rows_bytes() == N * 64 * -(-2 * d // 64), name
        return made[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_rows_do_not_depend_on_the_row_store(built, wa, name):
    """both register cores (beams 10 and 40 x 2 = 80) and the LDS-beam cores (200, 400) under windows of 2^-9, 2^-5, 2^-3 and all
    of the points, through the host, device, asynchronous and per-query-id calls; on d = 128 the one-wave core too (beam 2000
    on 50 queries)"""
    b = built(name)
    idx = b.idx
    try:
        for p in (-9, -5, -3, 0):
            W = windows(b.labels, NQ, p, 90 + p).astype(np.float32)
            for beam, mult in ((10, 1), (40, 2), (200, 1), (400, 1)):
                qp = _qp(wa, beam, mult)
                rows = {}
                for on in (False, True):
                    assert idx.set_half_rows(on) is on
                    for form in FORMS:
                        rows[on, form] = r = b.call(form, W, "optimized_postfilter", qp)
                        assert r[2]["half_rows"] == (1 if on else 0), (name, p, beam, form, on)
                        # (2^-9 of 30 000 points is 58 points: below the cutoff such a window is scanned, on the float32 rows)
                        assert r[2]["beam_searches"] > 0 or p == -9
                for form in FORMS:
                    _same(rows[True, form], rows[False, form], (name, p, beam, mult, form))
                    _same(rows[True, form], rows[False, "host"], (name, p, beam, mult, form, "vs host"))
        if CASES[name][0] == 128:
            nq = 50
            W = windows(b.labels, nq, 0, 91).astype(np.float32)
            rows = {}
            for on in (False, True):
                assert idx.set_half_rows(on) is on
                ids, dists = idx.batch_search(b.Q[:nq], W, nq, "optimized_postfilter", _qp(wa, 2000))
                rows[on] = (ids.copy(), dists.view(np.uint32).copy(), idx.counters())
                assert rows[on][2]["half_rows"] == (1 if on else 0) and rows[on][2]["beam_searches"] >= nq
            _same(rows[True], rows[False], (name, "beam 2000"))
    finally:
        idx.set_half_rows(True)  # (what a new index starts with)


@pytest.mark.parametrize("method", ["three_split", "fenwick"])
def test_multi_bucket_methods(built, wa, method):
    """their graph searches read the paired rows; their end scans the float32 rows, or, under set_scan_rows, the paired rows too"""
    b = built("d128_l2")
    idx = b.idx
    W = windows(b.labels, NQ, -5, 92).astype(np.float32)
    qp = _qp(wa, 40, 2)
    try:
        assert idx.set_half_rows(False) is False
        want = {form: b.call(form, W, method, qp) for form in ("host", "device")}
        assert idx.set_half_rows(True) is True
        for scan in (False, True):
            assert idx.set_scan_rows(scan) is scan
            for form in ("host", "device"):
                got = b.call(form, W, method, qp)
                assert got[2]["half_rows"] == 1 and got[2]["scan_rows"] == (1 if scan else 0), (method, form, scan)
                _same(got, want[form], (method, form, scan))
        assert want["host"][2]["brute_rows"] > 0 and want["host"][2]["beam_searches"] > 0
    finally:
        idx.set_scan_rows(False)
        idx.set_half_rows(True)


@pytest.mark.parametrize("name", SCAN_CASES)
def test_exact_scans_of_the_paired_rows(built, wa, name):
    """windows of 2^-12 .. 2^-9 of the points (7 .. 58: every query is an exact scan) with set_scan_rows on -- the plain k_brute
    of the new unit scores the paired rows -- against the float32 rows"""
    b = built(name)
    idx = b.idx
    qp = _qp(wa, 20)
    try:
        for p in (-12, -11, -10, -9):
            W = windows(b.labels, NQ, p, 93 + p).astype(np.float32)
            for form in ("host", "device"):
                assert idx.set_half_rows(False) is False and idx.set_scan_rows(False) is False
                off = b.call(form, W, "optimized_postfilter", qp)
                assert off[2]["scan_rows"] == 0 and off[2]["brute_rows"] > 0 and off[2]["beam_searches"] == 0, (name, p, form)
                assert idx.set_half_rows(True) is True and idx.set_scan_rows(True) is True
                on = b.call(form, W, "optimized_postfilter", qp)
                assert on[2]["scan_rows"] == 1, (name, p, form, on[2]["scan_rows"])
                _same(on, off, (name, "scan", p, form))
    finally:
        idx.set_scan_rows(False)
        idx.set_half_rows(True)


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_paired_rows_against_the_oracle(built, wa, oracle, name):
    """one batch of 100 queries from the paired rows against the CPU restatement: rows, searches and hops"""
    b = built(name)
    nq = 100
    oi = getattr(oracle, b.cls)(b.X, b.labels, build_params=oracle.BuildParams(32, 64, 1.0, b.idx_cache), **KW)
    W = windows(b.labels, nq, -3, 94)
    assert b.idx.set_half_rows(True) is True
    ids, dists = b.idx.batch_search(b.Q[:nq], W, nq, "optimized_postfilter", _qp(wa, 40, 2))
    c = b.idx.counters()
    eids, edists = oi.batch_search(b.Q[:nq], W, nq, "optimized_postfilter", _qp(oracle, 40, 2))
    ok, why = gu.same_rows(eids, edists, ids, dists, False, gu.RowContext(b.X, b.labels, b.Q[:nq], W, gu.metric_of(b.cls)))
    assert ok, (name, why)
    oc = oi.last_counters
    assert c["half_rows"] == 1
    assert c["beam_searches"] == oc["searches"] and c["hops"] == oc["hops"], name
    assert c["dist_cmps"] + c["brute_rows"] == oc["dist_cmps"], name
