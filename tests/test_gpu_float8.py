"""GPU: float8 point sets (include/wann.h WANN_DTYPE_F8 = 8, OCP E4M3) against the float32 path on the points rounded to float8.
Every finite E4M3 pattern widens exactly to one float32 value and the kernels score it in the float32 path's arithmetic, so
ids, distance bits and counters must equal those of the float32 index on the upcast rows -- through the scan, the beam search
and both ways a query reaches the device.  The rows are interleaved on the device (wann_byte_row_position); nothing of that
shows in a result."""
import numpy as np
import pytest

import golden_util as gu
from util import distinct_labels, repeated_labels, tie_windows, windows

pytestmark = pytest.mark.gpu
F8 = 8
PATTERNS = np.array([b for b in range(256) if (b & 0x7F) != 0x7F], dtype=np.uint8)  # the 254 finite patterns
OPS = ("beam_searches", "hops", "dist_cmps", "brute_rows", "label_reads", "spec_searches", "gemm_queries", "gemm_unproven", "gemm_rescued")


def _qp(mod, beam, mult=1, k=10, max_beam=10000):
    return mod.QueryParams(k, beam, 1.35, 10_000_000, 10_000, mult, max_beam, None, False)


def _decode_table():
    torch = pytest.importorskip("torch")
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()


def _device_search(torch, idx, Q, W, k, beam=10, mult=1, method=""):
    """one device-buffer call with fp32 queries (not rounded): (ids, dists)"""
    dev = torch.device("cuda:0")
    nq = len(Q)
    tq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    tw = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).to(dev)
    ti = torch.zeros((nq, k), dtype=torch.int32, device=dev)
    td = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    import window_ann
    idx.batch_search_device(tq.data_ptr(), tw.data_ptr(), nq, 0, method, _qp(window_ann, beam, mult, k), ti.data_ptr(), td.data_ptr(), 0)
    torch.cuda.synchronize()
    return ti.cpu().numpy().view(np.uint32), td.cpu().numpy()


def _pattern_rows(d):
    """254 points: element j of point i is the finite pattern i rotated by j -- every pattern in every element position"""
    i, j = np.arange(254)[:, None], np.arange(d)[None, :]
    return PATTERNS[(i + j) % 254]


def _fixed_queries(nq, d, seed):
    """non-trivial fp32 queries, NOT float8 values"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nq, d)) * np.float32(3.1) + np.float32(0.37)).astype(np.float32)


# ------------------------------------------------------------------------------------------
# every pattern through every fetch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ("Euclidian", "Mips"))
@pytest.mark.parametrize("d", (4, 36, 100))
def test_every_pattern_through_the_scan(wa, gpu, metric, d):
    """PrefilterIndex (k_brute on gathered rows), fp32 device queries, k = all 254 points: the distance bits of the float32 index
    on the upcast.  d = 36 and 100 cross a 32-element group and end in a ragged tail: interleave, quads, the odd last block."""
    torch = pytest.importorskip("torch")
    tab = _decode_table()
    bits = _pattern_rows(d)
    X = tab[bits]
    assert np.array_equal(wa.float8_bits(X), bits)
    labels = distinct_labels(254, 3)
    Q = _fixed_queries(24, d, 7 + d)
    W = np.tile(np.array([[-1.0, 2.0]]), (len(Q), 1))
    h = getattr(wa, "PrefilterIndexFloat8" + metric)(X, labels)
    f = getattr(wa, "PrefilterIndexFloat" + metric)(X, labels)
    hi, hd = _device_search(torch, h, Q, W, 254)
    fi, fd = _device_search(torch, f, Q, W, 254)
    assert np.array_equal(hd.view(np.uint32), fd.view(np.uint32))
    uniq = np.array([len(np.unique(r)) == len(r) for r in fd])
    assert np.array_equal(hi[uniq], fi[uniq])
    # every point the float32 index's window holds came back (the reference's window rule leaves the largest label out)
    assert all(sorted(a.tolist()) == sorted(b.tolist()) for a, b in zip(hi, fi))
    assert all(len(set(r.tolist())) >= 253 for r in hi)


def test_every_pattern_decodes_to_the_table(wa, gpu):
    """d = 4, unit queries under MIPS: every returned distance is minus the decode table's value of the element the query picks"""
    torch = pytest.importorskip("torch")
    tab = _decode_table()
    bits = _pattern_rows(4)
    X = tab[bits]
    labels = distinct_labels(254, 3)
    Q = np.eye(4, dtype=np.float32)
    W = np.tile(np.array([[-1.0, 2.0]]), (4, 1))
    h = wa.PrefilterIndexFloat8Mips(X, labels)
    ids, dists = _device_search(torch, h, Q, W, 253)  # (the reference's window rule leaves the point of the largest label out)
    seen = set()
    for j in range(4):
        got = bits[ids[j].astype(np.int64), j]
        want = -tab[got]
        assert np.array_equal(dists[j], want), j  # (values: -0.0 == 0.0)
        assert np.array_equal(np.sort(dists[j]), dists[j]) and len(set(ids[j].tolist())) == 253
        seen |= set(got.tolist())
    assert seen == set(PATTERNS.tolist())  # all 254 finite patterns were scored, each in some element position
    # the subnormals and 448 came through as themselves
    assert dists.min() == -448.0 and np.float32(2.0 ** -9) in np.abs(dists)


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("d", (4, 36, 100))
def test_every_pattern_through_the_beam_search(wa, gpu, metric, d):
    """raw_beam_search_typed (k_search) on a circulant graph of degree 64 -- the widest adjacency row of the ordinary cores, the
    whole set within two hops -- at a beam that holds all 254 points: ids, distance bits, hops and comparisons of the float32
    rows on the upcast"""
    tab = _decode_table()
    bits = _pattern_rows(d)
    X = tab[bits]
    n, deg = 254, 64
    rows = np.zeros((n, deg + 1), dtype=np.int32)
    rows[:, 0] = deg
    off = np.concatenate([np.arange(1, 33), -np.arange(1, 33)])
    rows[:, 1:] = (np.arange(n)[:, None] + off[None, :]) % n
    Q = _fixed_queries(16, d, 11 + d)
    qids = np.arange(len(Q), dtype=np.int64) + 10**6
    for beam in (8, 254):
        h = wa.raw_beam_search_typed(metric, F8, bits, rows, 0, Q, qids, beam)
        f = wa.raw_beam_search_typed(metric, 0, X, rows, 0, Q, qids, beam)
        for a, b, name in zip(h, f, ("ids", "dists", "sizes", "hops", "cmps")):
            a, b = np.asarray(a), np.asarray(b)
            if name == "dists":
                a, b = a.view(np.uint32), b.view(np.uint32)
            if name in ("ids", "dists"):  # (beyond a search's size the rows are not written)
                m = np.arange(a.shape[1])[None, :] < np.asarray(f[2])[:, None]
                a, b = np.where(m, a, 0), np.where(m, b, 0)
            assert np.array_equal(a, b), (beam, name)
        if beam == 254:
            assert (np.asarray(h[2]) == 254).all()
    with pytest.raises(RuntimeError, match="uint8"):
        wa.raw_beam_search_typed(metric, F8, X, rows, 0, Q, qids, 8)


# ------------------------------------------------------------------------------------------
# parity with the float32 index on the upcast
# ------------------------------------------------------------------------------------------
GRAPH_KINDS = (("VamanaRangeFilterTreeIndex", dict(cutoff=300, split_factor=2)),
               ("SuperOptimizedPostfilterTreeIndex", dict(cutoff=300, split_factor=2, shift_factor=0.5)),
               ("PostfilterVamanaIndex", dict()))
SCAN_KINDS = (("RangeFilterTreeIndex", dict(cutoff=300, split_factor=2)), ("PrefilterIndex", dict()))
DIMS = (4, 20, 33, 64, 100, 128, 200)  # one block, odd block count, partial quad, 25 blocks, the compile-time limit, the run-time routine
PARITY = [(kinds[(i + m) % len(kinds)], metric, d)
          for i, d in enumerate(DIMS) for m, metric in enumerate(("Euclidian", "Mips")) for kinds in (GRAPH_KINDS, SCAN_KINDS)]


def _spread_rows(wa, rng, n, d):
    """rows over the whole E4M3 range: per-row scales 2^-8 .. 2^6, so subnormals, -0.0 and +-448 all occur; float32 arrays of
    float8 values"""
    x = rng.standard_normal((n, d)) * np.exp2(rng.uniform(-8, 6, (n, 1)))
    x = np.clip(x, -448, 448).astype(np.float32)
    x[::97, 0] = 448.0
    x[1::97, -1] = -448.0
    x[2::97, 0] = -0.0
    x[3::97, -1] = np.float32(2.0 ** -9)
    return wa.float8_round(x)


@pytest.mark.parametrize("kind_kw,metric,d", PARITY, ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_float8_index_equals_float32_index(wa, gpu, tmp_path, kind_kw, metric, d):
    torch = pytest.importorskip("torch")
    kind, kw = kind_kw
    n, nq, k = 3000, 200, 10
    rng = np.random.default_rng(1000 + d)
    X = _spread_rows(wa, rng, n, d)
    assert np.array_equal(wa.float8_round(X).view(np.uint32), X.view(np.uint32))
    assert (np.abs(X)[X != 0] < 2.0 ** -6).any() and (np.abs(X) == 448).any() and np.signbit(X[X == 0]).any()
    Q = _fixed_queries(nq, d, d)           # fp32 device queries: not float8 values
    Qh = wa.float8_round(np.clip(Q, -448, 448))  # host calls take float8 queries
    labels = distinct_labels(n, 9)
    cache = str(tmp_path) + "/"
    bp = wa.BuildParams(32, 64, 1.0, cache)
    h = getattr(wa, kind + "Float8" + metric)(X, labels, build_params=bp, **kw)
    f = getattr(wa, kind + "Float" + metric)(X, labels, build_params=bp, **kw)  # (opens the graphs the float8 build wrote)
    row32, row8 = -(-d * 4 // 64) * 64, -(-d // 64) * 64
    assert f.device_bytes() - h.device_bytes() == n * (row32 - row8)
    tree = kind.endswith("RangeFilterTreeIndex")
    methods = ("optimized_postfilter", "fenwick", "three_split") if tree else ("",)
    empty = np.tile(np.array([[2.0, 3.0]]), (nq, 1))  # beyond every label
    batches = [empty] + [windows(labels, nq, p, 60 + p) for p in (-10, -8, -6, -4, -2, 0)]
    mixed = np.concatenate([b[i::7] for i, b in enumerate(batches)])[:nq]
    for method in methods:
        a = (method,) if tree else ()
        for W in batches + [mixed]:
            for beam, mult in ((10, 1), (64, 2)):
                fi, fd = f.batch_search(Qh, W, nq, *a, _qp(wa, beam, mult, k))
                fc = f.counters()
                hi, hd = h.batch_search(Qh, W, nq, *a, _qp(wa, beam, mult, k))
                hc = h.counters()
                assert np.array_equal(hd.view(np.uint32), fd.view(np.uint32)), ("host", method, beam)
                assert np.array_equal(hi, fi), ("host", method, beam)
                assert [hc[x] for x in OPS] == [fc[x] for x in OPS], ("host", method, beam, hc, fc)
            fi, fd = _device_search(torch, f, Q, W, k, 20, 2, method)
            fc = f.counters()
            hi, hd = _device_search(torch, h, Q, W, k, 20, 2, method)
            hc = h.counters()
            assert np.array_equal(hd.view(np.uint32), fd.view(np.uint32)) and np.array_equal(hi, fi), ("device", method)
            assert [hc[x] for x in OPS] == [fc[x] for x in OPS], ("device", method, hc, fc)
    if hasattr(h, "set_exact_windows"):
        assert h.set_exact_windows(512) == 0 and f.set_exact_windows(512) == 0
        for W in (batches[3], batches[5], mixed):
            fi, fd = _device_search(torch, f, Q, W, k, 20, 2, methods[0])
            fc, fe = f.counters(), f.exact_window_counters()
            hi, hd = _device_search(torch, h, Q, W, k, 20, 2, methods[0])
            hc, he = h.counters(), h.exact_window_counters()
            assert np.array_equal(hd.view(np.uint32), fd.view(np.uint32)) and np.array_equal(hi, fi)
            assert he == fe and [hc[x] for x in OPS] == [fc[x] for x in OPS], (he, fe)
        assert fe["queries"] > 0


# ------------------------------------------------------------------------------------------
# further cases
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (4, 32))
@pytest.mark.parametrize("kind,kw", [("PrefilterIndex", dict()), ("VamanaRangeFilterTreeIndex", dict(cutoff=300, split_factor=2))])
@pytest.mark.parametrize("metric", ("Euclidian", "Mips"))
def test_float8_ties(oracle, wa, gpu, tmp_path, metric, kind, kw, d):
    """values in {-1, 0, 1} and repeated labels: nearly every distance is shared.  Distance bits equal the float32 index's, rows
    equal the oracle's up to its ties."""
    n, nq = 3000, 120
    rng = np.random.default_rng(17 + d)
    X = rng.integers(-1, 2, (n, d)).astype(np.float32)
    Q = rng.integers(-1, 2, (nq, d)).astype(np.float32)
    Q[::4] = X[rng.choice(n, len(Q[::4]))]
    assert np.array_equal(wa.float8_round(X), X)
    labels = repeated_labels(n, 31, 150)
    cache = str(tmp_path) + "/"
    h = getattr(wa, kind + "Float8" + metric)(X, labels, build_params=wa.BuildParams(32, 64, 1.0, cache), **kw)
    f = getattr(wa, kind + "Float" + metric)(X, labels, build_params=wa.BuildParams(32, 64, 1.0, cache), **kw)
    oi = getattr(oracle, kind + "Float" + metric)(X, labels, build_params=oracle.BuildParams(32, 64, 1.0, cache), **kw)
    tree = kind != "PrefilterIndex"
    a = ("optimized_postfilter",) if tree else ()
    for p in (-7, -3, -1):  # (tie_windows draws a start below n - w: the fraction stays below the whole set)
        W = tie_windows(labels, nq, p, 50 + p)
        hi, hd = h.batch_search(Q, W, nq, *a, _qp(wa, 40))
        fi, fd = f.batch_search(Q, W, nq, *a, _qp(wa, 40))
        assert np.array_equal(hd.view(np.uint32), fd.view(np.uint32)), p
        if tree and p > -7:  # (beam searches: the same order of the same candidates)
            assert np.array_equal(hi, fi), p
        eids, edists = oi.batch_search(Q, W, nq, *a, _qp(oracle, 40))
        ctx = gu.RowContext(X, labels, Q, W, gu.metric_of(metric), *(() if tree else ("prefilter",)))
        ok, why = gu.same_rows(eids, edists, hi, hd, True, ctx)
        assert ok, f"{kind}Float8{metric} d={d} p={p}: {why}"


def test_float8_async_lanes_return_the_blocking_rows(wa, gpu, tmp_path):
    torch = pytest.importorskip("torch")
    n, nq, d, k = 3000, 200, 100, 10
    rng = np.random.default_rng(3)
    X = _spread_rows(wa, rng, n, d)
    Q = _fixed_queries(nq, d, 5)
    labels = distinct_labels(n, 2)
    h = wa.VamanaRangeFilterTreeIndexFloat8Mips(X, labels, cutoff=300, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/"))
    dev = torch.device("cuda:0")
    tq = torch.from_numpy(Q).to(dev)
    qp = _qp(wa, 20, 2, k)
    Ws = [windows(labels, nq, p, 80 + p).astype(np.float32) for p in (-8, -4, -1)]
    want = [_device_search(torch, h, Q, W, k, 20, 2, "optimized_postfilter") for W in Ws]
    tws = [torch.from_numpy(W).to(dev) for W in Ws]
    outs = [(torch.zeros((nq, k), dtype=torch.int32, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev)) for _ in Ws]
    torch.cuda.synchronize()
    tickets = [h.batch_search_device_async(tq.data_ptr(), tw.data_ptr(), nq, 0, "optimized_postfilter", qp, ti.data_ptr(), td.data_ptr(), 0)
               for tw, (ti, td) in zip(tws, outs)]
    for t in tickets:
        h.wait(t)
    for (ti, td), (wi, wd) in zip(outs, want):
        assert np.array_equal(ti.cpu().numpy().view(np.uint32), wi) and np.array_equal(td.cpu().numpy().view(np.uint32), wd.view(np.uint32))


def test_float8_nan_patterns_are_refused_and_no_shadow_rows(wa, gpu):
    n, d = 500, 20
    rng = np.random.default_rng(1)
    X = wa.float8_round(rng.standard_normal((n, d)).astype(np.float32))
    labels = distinct_labels(n, 1)
    for bad in (1000.0, 465.0, np.inf, np.nan, -1e9):
        Y = X.copy()
        Y[123, 7] = bad
        with pytest.raises(RuntimeError, match="row 123"):
            wa.PrefilterIndexFloat8Euclidian(Y, labels)
    h = wa.PostfilterVamanaIndexFloat8Euclidian(X, labels, build_params=wa.BuildParams(16, 32, 1.0, ""))
    Q = X[:8].copy()
    W = np.tile(np.array([[-1.0, 2.0]]), (8, 1))
    h.batch_search(Q, W, 8, _qp(wa, 10))
    Q[5, 3] = 1e6
    with pytest.raises(RuntimeError, match="query row 5"):
        h.batch_search(Q, W, 8, _qp(wa, 10))
    # no shadow copies: the getters say so and the setters leave everything off
    assert (h.half_rows(), h.byte_rows(), h.scan_rows(), h.dense_rows()) == (False,) * 4
    assert (h.half_rows_bytes(), h.byte_rows_bytes(), h.dense_rows_bytes()) == (0, 0, 0)
    assert (h.set_half_rows(True), h.set_byte_rows(True), h.set_scan_rows(True), h.set_dense_rows(True)) == (False,) * 4
    assert h.device_bytes() > 0
