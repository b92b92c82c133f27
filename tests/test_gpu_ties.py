"""GPU: exact distance ties and repeated labels against the oracle.  Small-range integer rows (the normal case of uint8 / int8
point sets) give most candidates a distance that other candidates share, and repeated labels put window ends inside runs of
equal labels.  The reference rejects a candidate whose distance EQUALS the beam's cutoff (beamSearch.h:135-145), sorts equal
keys in a fixed way, and bounds windows with lower bounds on the sorted labels (tree_utils.h:19-37, prefiltering.h:159-184);
a kernel that gets any of this wrong still returns plausible rows, so every comparison here is bit-exact: ids, distance bits,
hops and dist_cmps -- tie-aware only for the rows that the reference itself answers with an exact scan or a merged list."""
import os

import numpy as np
import pytest

import golden_util as gu
from util import repeated_labels, distinct_labels, sift_like, tie_heavy, tie_queries, tie_windows, windows

pytestmark = pytest.mark.gpu
U8, I8 = 1, 2
ELEM = {U8: np.uint8, I8: np.int8}
THREADS = min(16, os.cpu_count() or 1)


def _as_elem(sfx, a):
    """a as the index of class suffix sfx holds it (py::array_t<T> forcecast: numpy's cast), back in float32"""
    for name, t in (("UInt8", np.uint8), ("Int8", np.int8)):
        if sfx.startswith(name):
            return np.asarray(a).astype(t).astype(np.float32)
    return a


def _qp(mod, beam, mult=1, k=10, max_beam=10000):
    return mod.QueryParams(k, beam, 1.35, 10_000_000, 10_000, mult, max_beam, None, False)


def _raw_mismatches(oracle_rows, got):
    ids, dists, sizes, hops, cmps = got
    bad = []
    for i, (oi, od, nv, dc) in enumerate(oracle_rows):
        m = int(sizes[i])
        if not (m == len(oi) and np.array_equal(ids[i, :m], oi) and np.array_equal(dists[i, :m].view(np.uint32), od.view(np.uint32))
                and int(hops[i]) == nv and int(cmps[i]) == dc):
            bad.append((i, m, len(oi), int(hops[i]), nv, int(cmps[i]), dc))
    return bad


def _oracle_raw(oracle, rows, Xp, d, metric, start, Q, qids, beam):
    out = []
    for i in range(len(Q)):
        oi, od, vi, _, dc = oracle.beam_search(rows, Xp, d, metric | oracle.INTEGER, start, Q[i], int(qids[i]), beam)
        out.append((oi, od, len(vi), dc))
    return out


# ------------------------------------------------------------------------------------------
# 1. every beam-search core of the byte translation units on tie-heavy rows
# ------------------------------------------------------------------------------------------
RAW_BEAMS = (1, 7, 64, 65, 128, 129, 130, 320, 1280, 1281, 2500)  # (both sides of every core boundary)
_CORES = [{}, {"WANN_FORCE_GENERAL": "1"}, {"WANN_OLD_GENERAL": "1"}, {"WANN_RAW_BIG_LDS": "1"},
          {"WANN_RAW_BIG_LDS": "1", "WANN_FORCE_GENERAL": "1"}]
CORE_VARIANTS = _CORES + [dict(e, WANN_NO_HELPER="1") for e in _CORES]
_raw_cache = {}


def _raw_tie_case(oracle, dtype, metric):
    """data, graph and the oracle's rows of one (dtype, metric) at every beam: computed once, reused by every core variant"""
    key = (dtype, metric)
    if key not in _raw_cache:
        n, nq, R, L, d = 4000, 48, 32, 64, 6
        lo, hi = (0, 12) if dtype == U8 else (-6, 6)
        X = tie_heavy(n, d, 99 + dtype, lo, hi, dup_frac=0.15, zero_rows=64)
        Q = tie_queries(X, nq, 7 + dtype, lo, hi)
        Xp = oracle.pad_rows(X)
        start, sn = 200, 3600
        rows = oracle.vamana_build(Xp, d, metric | oracle.INTEGER, start, sn, R, L, 1.0, THREADS)
        qids = np.arange(nq, dtype=np.int64) + 10**6
        qids[1::6] = np.arange(1, nq, 6) * 37  # (some queries carry the id of a node: the self-skip quirk)
        want = {beam: _oracle_raw(oracle, rows, Xp, d, metric, start, Q, qids, beam) for beam in RAW_BEAMS}
        _raw_cache[key] = (X.astype(ELEM[dtype]), Q, rows, start, qids, want)
    return _raw_cache[key]


@pytest.mark.parametrize("env", CORE_VARIANTS, ids=lambda e: "+".join(sorted(e)) or "default")
@pytest.mark.parametrize("dtype,metric", [(U8, 0), (U8, 1), (I8, 0), (I8, 1)], ids=["u8-l2", "u8-mips", "i8-l2", "i8-mips"])
def test_raw_byte_cores_on_tie_heavy_data(oracle, wa, gpu, monkeypatch, env, dtype, metric):
    """d = 6 rows of the values 0..11 (uint8) / -6..5 (int8), 15 % duplicated rows and a block of all-zero rows; a quarter of
    the queries are points and one is all zero (under MIPS every distance to it is -0.0: the whole graph is one tie group).
    raw_beam_search_typed against the oracle's int32 accumulation, in every core, at beams on both sides of every core boundary."""
    Xb, Q, rows, start, qids, want = _raw_tie_case(oracle, dtype, metric)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    bad = []
    for beam in RAW_BEAMS:
        got = wa.raw_beam_search_typed(metric, dtype, Xb, rows, start, Q, qids, beam)
        bad += [(beam,) + b for b in _raw_mismatches(want[beam], got)]
    assert not bad, (len(bad), bad[:8])


# ------------------------------------------------------------------------------------------
# 2. byte row shapes: partial last query word, 64-byte row padding, chunk counts that are no multiple of 8
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 4, 5, 15, 17, 63, 64, 65, 127, 129, 1024])
@pytest.mark.parametrize("dtype,metric", [(U8, 0), (U8, 1), (I8, 0), (I8, 1)], ids=["u8-l2", "u8-mips", "i8-l2", "i8-mips"])
def test_raw_byte_row_shapes(oracle, wa, gpu, dtype, metric, d):
    n, nq, R, L = 1200, 32, 16, 32
    g = sift_like(n, d, 40 + d)
    shift = 0.0 if dtype == U8 else 128.0
    X = (g(n) - shift).astype(ELEM[dtype]).astype(np.float32)
    Q = (g(nq) - shift).astype(ELEM[dtype]).astype(np.float32)
    Xp = oracle.pad_rows(X)
    start, sn = 100, 1000
    rows = oracle.vamana_build(Xp, d, metric | oracle.INTEGER, start, sn, R, L, 1.0, THREADS)
    qids = np.arange(nq, dtype=np.int64) + 10**6
    bad = []
    for beam in (10, 100, 700):
        got = wa.raw_beam_search_typed(metric, dtype, X.astype(ELEM[dtype]), rows, start, Q, qids, beam)
        bad += [(beam,) + b for b in _raw_mismatches(_oracle_raw(oracle, rows, Xp, d, metric, start, Q, qids, beam), got)]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("sfx", ["UInt8Euclidian", "Int8Mips"])
def test_float_queries_on_byte_indexes_cast_like_numpy(oracle, wa, gpu, tmp_path, sfx):
    """Queries handed over as float32 with fractional values, negative values (uint8) and values above 127 (int8), all inside
    the int32 range: the reference's py::array_t<T> forcecast converts them as numpy does (truncate, keep the low byte)."""
    n, d, nq = 3000, 16, 200
    g = sift_like(n, d, 8)
    X = g(n) if sfx.startswith("UInt8") else g(n) - 128.0
    rng = np.random.default_rng(4)
    Q = (g(nq) - 128.0 + rng.uniform(-1, 1, (nq, d)) * 3).astype(np.float32)  # fractional, negative
    Q[::3] += 160.0                                                           # above 127 and above 255
    Q[1::7] *= 1000.0                                                         # far outside the byte range
    labels = distinct_labels(n, 9)
    cache = str(tmp_path) + "/"
    kw = dict(cutoff=400, split_factor=2)
    pi = getattr(wa, "VamanaRangeFilterTreeIndex" + sfx)(X, labels, build_params=wa.BuildParams(24, 48, 1.0, cache), **kw)
    oi = getattr(oracle, "VamanaRangeFilterTreeIndex" + sfx)(X, labels, build_params=oracle.BuildParams(24, 48, 1.0, cache),
                                                            threads=THREADS, **kw)
    for p, method, beam in ((-2, "optimized_postfilter", 20), (-8, "optimized_postfilter", 10), (-4, "fenwick", 20)):
        W = windows(labels, nq, p, 5 - p)
        ids, dists = pi.batch_search(Q, W, nq, method, _qp(wa, beam))
        eids, edists = oi.batch_search(Q, W, nq, method, _qp(oracle, beam))
        exact = gu.exact_rows("VamanaRangeFilterTreeIndex", method, labels, W, 400)
        ctx = gu.RowContext(X, labels, _as_elem(sfx, Q), W, gu.metric_of(sfx), gu.window_rule("VamanaRangeFilterTreeIndex", method))
        ok, why = gu.same_rows(eids, edists, ids, dists, exact, ctx)
        assert ok, (p, method, why)


# ------------------------------------------------------------------------------------------
# 3. index level: every kind on one index per dataset, distinct and repeated labels, alternating launch shapes
# ------------------------------------------------------------------------------------------
N_IDX, CUTOFF = 20000, 400
DATASETS = {  # name: (class suffix, value range, all-zero rows)
    "f32-l2": ("FloatEuclidian", (0, 12), 0),
    "u8-l2": ("UInt8Euclidian", (0, 12), 0),
    "i8-mips": ("Int8Mips", (-6, 6), 200),
}
LABELS = {"distinct": lambda n: distinct_labels(n, 31), "repeated": lambda n: repeated_labels(n, 31, 150)}
INDEX_KINDS = [("VamanaRangeFilterTreeIndex", ("optimized_postfilter", "fenwick", "three_split")),
               ("SuperOptimizedPostfilterTreeIndex", (None,)), ("PostfilterVamanaIndex", (None,)),
               ("RangeFilterTreeIndex", ("optimized_postfilter", "fenwick", "three_split")), ("PrefilterIndex", (None,))]
# (fraction 2^p, beam, final_beam_multiply, queries): launch shapes alternate on one index, and the postfilter chains double
# across the 128 and 1 280 boundaries; 2^-9 windows are fenwick_tree_search's in optimized_postfiltering_search (4 w < cutoff)
SCHEDULE = [(-3, 2000, 1, 7), (-6, 80, 2, 300), (-5, 2000, 4, 1), (-3, 10, 1, 3000), (-7, 10, 1, 300), (-4, 40, 3, 300),
            (-9, 20, 2, 300), (-5, 20, 4, 7)]


def _index_pair(oracle, wa, tmp_path, kind, sfx, X, labels):
    cache = str(tmp_path) + "/"
    kw = dict(cutoff=CUTOFF, split_factor=2) if "Tree" in kind else {}
    if kind.startswith("Super"):
        kw = dict(cutoff=CUTOFF, split_factor=2, shift_factor=0.5)
    labkw = "filters" if kind == "PostfilterVamanaIndex" else "filter_values"
    pi = getattr(wa, kind + sfx)(X, **{labkw: labels}, build_params=wa.BuildParams(24, 48, 1.0, cache), **kw)
    oi = getattr(oracle, kind + sfx)(X, **{labkw: labels}, build_params=oracle.BuildParams(24, 48, 1.0, cache), threads=THREADS, **kw)
    return pi, oi


def _check_call(pi, oi, wa, oracle, kind, sfx, method, X, labels, Q, W, beam, mult, what):
    nq = len(Q)
    a = (Q, W, nq) + ((method,) if method else ())
    ids, dists = pi.batch_search(*a, _qp(wa, beam, mult))
    eids, edists = oi.batch_search(*a, _qp(oracle, beam, mult))
    c, oc = pi.counters(), oi.last_counters
    exact = gu.exact_rows(kind, method, labels, W, CUTOFF)
    rule = gu.window_rule(kind, method)
    cands = gu.oracle_candidates(oi, Q, W, method, lambda k: _qp(oracle, beam, mult, k)) if rule == "candidates" else None
    ctx = gu.RowContext(X, labels, _as_elem(sfx, Q), W, gu.metric_of(sfx), rule, cands)
    ok, why = gu.same_rows(eids, edists, ids, dists, exact, ctx)
    assert ok, f"{kind}{sfx} {method} {what}: {why}"
    assert (c["beam_searches"], c["hops"]) == (oc["searches"], oc["hops"]), (what, c, oc)
    if c["gemm_queries"] == 0:  # (float32 PrefilterIndex batches whose windows repeat may take the dense path: it scans no rows)
        assert c["dist_cmps"] + c["brute_rows"] == oc["dist_cmps"], (what, c, oc)


@pytest.mark.parametrize("kind,methods", INDEX_KINDS, ids=[k for k, _ in INDEX_KINDS])
@pytest.mark.parametrize("labs", list(LABELS))
@pytest.mark.parametrize("data", list(DATASETS))
def test_index_ties_and_repeated_labels(oracle, wa, gpu, tmp_path, data, labs, kind, methods):
    """n = 20 000 rows of d = 6 small integers; distinct labels, or about 150 label values in runs of about 130 points (runs
    straddle partition boundaries at cutoff 400).  With repeated labels the windows include [v, v] (zero width in the sorted
    order, though a whole run carries v), both ends inside runs, hi equal to the largest label and lo below the smallest.  One
    index takes every call, launch shapes alternating; rows and work counters equal the oracle's."""
    sfx, (lo, hi), zeros = DATASETS[data]
    X = tie_heavy(N_IDX, 6, 5, lo, hi, dup_frac=0.15, zero_rows=zeros)
    Qall = tie_queries(X, 3000, 6, lo, hi)
    labels = LABELS[labs](N_IDX)
    pi, oi = _index_pair(oracle, wa, tmp_path, kind, sfx, X, labels)
    for step, (p, beam, mult, nq) in enumerate(SCHEDULE):
        Q = Qall[:nq] if step % 2 == 0 else Qall[-nq:]
        W = tie_windows(labels, nq, p, 60 + step)
        for method in methods:
            _check_call(pi, oi, wa, oracle, kind, sfx, method, X, labels, Q, W, beam, mult, f"step {step} p={p} beam={beam}x{mult} nq={nq}")


def _dense_windows(labels, nq, seed):
    """windows shared by groups of 20 queries, each of 1 024 .. 6 000 points, ends from the sorted labels (inside runs where
    labels repeat); every tenth query has a window of its own"""
    rng = np.random.default_rng(seed)
    s = np.sort(labels)
    n = len(s)
    W = np.zeros((nq, 2))
    for g0 in range(0, nq, 20):
        w = int(rng.integers(1100, 6000))
        st = int(rng.integers(0, n - w))
        W[g0:g0 + 20] = (s[st], s[st + w])
    W[-20:] = (s[-3000], s[-1])        # hi = the largest label
    W[-40:-20] = (s[0] - 1, s[2500])   # lo below the smallest label
    for i in range(5, nq, 10):
        st = int(rng.integers(0, n - 300))
        W[i] = (s[st], s[st + int(rng.integers(0, 300))])
    return W


@pytest.mark.parametrize("labs", list(LABELS))
def test_dense_prefilter_ties_and_repeated_labels(oracle, wa, gpu, monkeypatch, labs):
    """PrefilterIndex on d = 24 small integers (exact in bf16: every tie is exact inside k_gemm_scores too), groups of 20 queries
    sharing windows of more than 1 024 points: the dense path (WANN_DENSE_ALWAYS) and the exact scan (WANN_NO_GEMM) both return
    the oracle's rows, and the same rows as each other.  Then a batch in which every third query's window is empty and no two
    windows are alike: the dense path, tried on it, must leave exactly the oracle's exact-scan work -- an empty window emits no
    task, and its task slot must not offer the dense path the window of the batch before."""
    n, d, nq = N_IDX, 24, 400
    X = tie_heavy(n, d, 12, 0, 12, dup_frac=0.15)
    Q = tie_queries(X, nq, 13, 0, 12)
    labels = LABELS[labs](n)
    W = _dense_windows(labels, nq, 3)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    pi = wa.PrefilterIndexFloatEuclidian(X, labels)
    oi = oracle.PrefilterIndexFloatEuclidian(X, labels, threads=THREADS)
    ctx = gu.RowContext(X, labels, Q, W, "l2", "prefilter")
    rows = []
    for k, gemm in ((10, True), (10, False), (16, True)):
        if gemm:
            monkeypatch.delenv("WANN_NO_GEMM", raising=False)
        else:
            monkeypatch.setenv("WANN_NO_GEMM", "1")
        ids, dists = pi.batch_search(Q, W, nq, _qp(wa, 10, 1, k))
        c = pi.counters()
        assert (c["gemm_queries"] > nq // 2) if gemm else (c["gemm_queries"] == 0), c
        eids, edists = oi.batch_search(Q, W, nq, _qp(oracle, 10, 1, k))
        ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
        assert ok, f"k={k} gemm={gemm}: {why}"
        if not gemm:
            assert c["dist_cmps"] + c["brute_rows"] == oi.last_counters["dist_cmps"], (c, oi.last_counters)
        rows.append((ids, dists))
    assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1])
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    s = np.sort(labels)
    rng = np.random.default_rng(8)
    W2 = np.zeros((nq, 2))
    for i in range(nq):
        st = int(rng.integers(0, n - 400))
        W2[i] = (s[st], s[st]) if i % 3 == 0 else (s[st], s[st + 30 + i % 97 + int(rng.integers(0, 200))])
    ids, dists = pi.batch_search(Q, W2, nq, _qp(wa, 10, 1, 10))
    c = pi.counters()
    eids, edists = oi.batch_search(Q, W2, nq, _qp(oracle, 10, 1, 10))
    ok, why = gu.same_rows(eids, edists, ids, dists, True, gu.RowContext(X, labels, Q, W2, "l2", "prefilter"))
    assert ok, why
    assert c["gemm_queries"] == 0 and c["dist_cmps"] + c["brute_rows"] == oi.last_counters["dist_cmps"], (c, oi.last_counters)
