"""GPU: uint8 / int8 rows of 513 .. 2048 bytes on the dense paths (`k_gemm_scores_bslab`).

The score kernel walks such a row in a run-time number of 256-byte slabs (the last one shorter, in multiples of 64 bytes), both
operands staged per slab, and hands over keys that hold the distance quantised to multiples of four (a lower bound).  The row
lengths here are the chunk counts and last-slab shapes at which such a loop goes wrong; n is the smallest at which a window
spans two position blocks and ends in a ragged step.  Per case:
  1. under WANN_NO_GEMM the batch runs on the exact scan alone (dense counters zero);
  2. the dense path's rows are the scan's, ids and distance bits, row for row;
  3. the scan's rows are the oracle's PrefilterIndex rows (distances bit for bit, ids up to exact ties);
  4. every eligible query is counted on its path (zero for these lengths before the kernel existed);
  5. at most a tenth of the batch is unproven on uniform random bytes -- a kernel that settles nothing would otherwise pass on
     the scan's rows.  (A numpy model of the selection -- keys quantised with S = 2, four smallest per 64 positions, 32
     selected, strict bound -- gives 0 unproven and at most 2 rescued of 192 such queries, for both types and metrics.)
Counters are printed per case and appended to $DENSE_LONG_BYTES_COUNTERS_OUT when set."""
import os

import numpy as np
import pytest

import golden_util as gu
import numerics_util as nu

pytestmark = pytest.mark.gpu

ZERO = dict(queries=0, unproven=0, rescued=0, groups=0, tiles=0, passes=0, handover_bytes=0)
BLOCK = nu.BLOCK
N = 3 * BLOCK + 64
F, REP = 6, nu.REP
# 513 pads to 576: the first length past k_gemm_scores_b, two full slabs and one of 64 bytes; 640: exactly ten chunks; 1000 pads to
# 1024: four full slabs; 1025 pads to 1088: one chunk past a slab boundary; 1536: six full slabs; 2048: the limit
DIMS = (513, 640, 1000, 1025, 1536, 2048)
SFX = ("UInt8Euclidian", "UInt8Mips", "Int8Euclidian", "Int8Mips")


def _qp(mod, k=10):
    return mod.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def _note(line):
    print("[dense long bytes] " + line)
    out = os.environ.get("DENSE_LONG_BYTES_COUNTERS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _elem(sfx):
    return np.uint8 if sfx.startswith("UInt8") else np.int8


def _range(elem):
    return (0, 255) if elem == np.uint8 else (-128, 127)


def _rows(rng, elem, n, d, kind):
    lo, hi = _range(elem)
    if kind == "ties":  # three values: many equal distances
        return rng.integers(lo + 126, lo + 129, (n, d)).astype(elem)
    return rng.integers(lo, hi + 1, (n, d)).astype(elem)


class _Batch:
    """N rows of uniform random bytes with distinct labels in a random order, and F families of REP queries.  Family f shares the
    window [a_f, b_f) of 1 700 .. 3 000 positions (even f: a_f a multiple of 128, odd f: not); on the cover path query j of the
    family has [a_f + j, b_f - j).  The ends are drawn so that all REP windows of a family touch the same position blocks: every
    block a query touches then has at least REP >= 32 wide queries, and every query is eligible for the cover path.  No window
    reaches the last 64 positions (the reference's scan never returns the last point).
    kind "extremes": eight rows at each end of the element range (all 255 / all 0; int8: all 127 / all -128) lie inside every
    family's window, and four queries of every family are constant at each end; kind "ties": elements from three values."""

    def __init__(self, d, elem, kind="uniform"):
        rng = np.random.default_rng(8000 + d + (0 if elem == np.uint8 else 1))
        self.d, self.elem = d, elem
        self.X = _rows(rng, elem, N, d, kind)
        self.Q = _rows(rng, elem, F * REP, d, kind)
        self.order = rng.permutation(N)  # order[pos] = the row at position pos of the label argsort
        self.labels = np.empty(N, dtype=np.float32)
        self.labels[self.order] = np.arange(N, dtype=np.float32)
        a, b = np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int64)
        for f in range(F):
            while True:
                w = int(rng.integers(1700, 3001))
                s = int(rng.integers(0, N - 64 - w + 1))
                s = s - s % 128 if f % 2 == 0 else s | 1
                e = s + w
                if e <= N - 64 and w % 128 and s // BLOCK == (s + REP - 1) // BLOCK and (e - REP) // BLOCK == (e - 1) // BLOCK:
                    break
            a[f], b[f] = s, e
        assert ((a // BLOCK) != ((b - 1) // BLOCK)).any() and (b - a > BLOCK).any()  # two position blocks; two slices of a window
        self.a, self.b = a, b
        self.family = np.repeat(np.arange(F), REP)
        if kind == "extremes":
            lo, hi = _range(elem)
            for f in range(F):
                pos = rng.choice(np.arange(a[f], b[f]), 16, replace=False)
                self.X[self.order[pos[:8]]] = hi
                self.X[self.order[pos[8:]]] = lo
                self.Q[f * REP:f * REP + 4] = hi
                self.Q[f * REP + 4:f * REP + 8] = lo
        self._oracle = {}

    def windows(self, path):
        j = np.tile(np.arange(REP), F) if path == "cover" else 0
        a, b = self.a[self.family] + j, self.b[self.family] - j
        return np.stack([a - 0.5, b - 0.5], 1).astype(np.float64)

    def oracle_rows(self, oracle, sfx, path, k):
        """the oracle's PrefilterIndex rows of the batch, computed once"""
        key = (sfx, path, k)
        if key not in self._oracle:
            oi = getattr(oracle, "PrefilterIndex" + sfx)(self.X, self.labels)
            self._oracle[key] = oi.batch_search(self.Q, self.windows(path), len(self.Q), _qp(oracle, k))
        return self._oracle[key]

    def context(self, sfx, W):
        return gu.RowContext(self.X.astype(np.float32), self.labels, self.Q.astype(np.float32), W, gu.metric_of(sfx), "prefilter")


_batches, _indexes = {}, {}


def _batch(d, elem, kind="uniform"):
    if (d, elem, kind) not in _batches:
        _batches.clear()  # (one row length and element type at a time)
        _indexes.clear()
        _batches[d, elem, kind] = _Batch(d, elem, kind)
    return _batches[d, elem, kind]


def _index(wa, sfx, bt):
    if sfx not in _indexes:
        _indexes[sfx] = getattr(wa, "PrefilterIndex" + sfx)(bt.X, bt.labels)
    return _indexes[sfx]


def _counters(pi, path):
    c, w = pi.counters(), pi.dense_window_counters()
    if path == "cover":
        assert c["gemm_queries"] == 0, c
        return dict(queries=w["queries"], unproven=w["unproven"], rescued=w["rescued"])
    assert w == ZERO, w
    return dict(queries=c["gemm_queries"], unproven=c["gemm_unproven"], rescued=c["gemm_rescued"])


def _scan_and_dense(pi, wa, monkeypatch, path, Q, W, k, long_rows=True):
    """the batch on the exact scan (dense counters zero), then on the dense path `path`: rows equal bit for bit.  Returns the
    scan's rows and the path's counters."""
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work for the cover path)
    if long_rows:
        monkeypatch.setenv("WANN_DENSE_LONG_ROWS", "1")  # (rows of more than 512 bytes take the dense path where the process opts in)
    else:
        monkeypatch.delenv("WANN_DENSE_LONG_ROWS", raising=False)
    nq = len(Q)
    pi.set_dense_windows(False)
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    ids0, d0 = pi.batch_search(Q, W, nq, _qp(wa, k))
    assert pi.counters()["gemm_queries"] == 0 and pi.dense_window_counters() == ZERO
    monkeypatch.delenv("WANN_NO_GEMM")
    pi.set_dense_windows(path == "cover")
    ids1, d1 = pi.batch_search(Q, W, nq, _qp(wa, k))
    ctr = _counters(pi, path)
    pi.set_dense_windows(False)
    bad = np.nonzero((d0.view(np.uint32) != d1.view(np.uint32)).any(axis=1) | (ids0 != ids1).any(axis=1))[0]
    assert len(bad) == 0, (path, k, len(bad), bad[:5], ids0[bad[:2]], ids1[bad[:2]], d0[bad[:2]], d1[bad[:2]], ctr)
    return ids0, d0, ctr


def _case(oracle, wa, monkeypatch, sfx, d, path, k=10):
    bt = _batch(d, _elem(sfx))
    pi = _index(wa, sfx, bt)
    W = bt.windows(path)
    ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, path, bt.Q, W, k)
    eids, edists = bt.oracle_rows(oracle, sfx, path, k)
    ok, why = gu.same_rows(eids, edists, ids, dists, True, bt.context(sfx, W))
    assert ok, f"{sfx} d={d} {path} k={k}: {why}"
    _note(f"{sfx} d={d} {path} k={k}: {ctr}")
    assert ctr["queries"] == len(bt.Q), (sfx, d, path, ctr)  # every query of these batches is eligible for its path
    assert ctr["unproven"] <= len(bt.Q) // 10, (sfx, d, path, ctr)
    return ids, dists, ctr


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d", DIMS)
def test_shared_windows(oracle, wa, gpu, monkeypatch, sfx, d):
    _case(oracle, wa, monkeypatch, sfx, d, "shared")


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d", (513, 1025, 2048))
def test_cover_groups(oracle, wa, gpu, monkeypatch, sfx, d):
    _case(oracle, wa, monkeypatch, sfx, d, "cover")


@pytest.mark.parametrize("sfx", SFX)
def test_key_range_extremes(oracle, wa, gpu, monkeypatch, sfx):
    """d = 2048: rows and queries at both ends of the element range beside random ones -- the largest and smallest distances a
    key has to hold (L2 0 and 255^2 x 2048; inner products -255^2 x 2048, -2^25 and 128 x 127 x 2048): a wrong offset or shift
    wraps a key here.  Rows equal the scan's and the oracle's."""
    d = 2048
    bt = _batch(d, _elem(sfx), "extremes")
    pi = _index(wa, sfx, bt)
    W = bt.windows("shared")
    ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, "shared", bt.Q, W, 10)
    _note(f"extremes {sfx} d={d} shared k=10: {ctr}")
    assert ctr["queries"] == len(bt.Q), ctr
    eids, edists = bt.oracle_rows(oracle, sfx, "shared", 10)
    ok, why = gu.same_rows(eids, edists, ids, dists, True, bt.context(sfx, W))
    assert ok, f"{sfx}: {why}"


@pytest.mark.parametrize("sfx", SFX)
def test_ties(oracle, wa, gpu, monkeypatch, sfx):
    """d = 576, elements from three values: distances tie in crowds, and only the scan's id order settles them.  Rows equal the
    scan's (no cap on unproven queries here)."""
    d = 576
    bt = _batch(d, _elem(sfx), "ties")
    pi = _index(wa, sfx, bt)
    W = bt.windows("shared")
    ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, "shared", bt.Q, W, 10)
    _note(f"ties {sfx} d={d} shared k=10: {ctr}")
    assert ctr["queries"] == len(bt.Q), ctr
    eids, edists = bt.oracle_rows(oracle, sfx, "shared", 10)
    ok, why = gu.same_rows(eids, edists, ids, dists, True, bt.context(sfx, W))
    assert ok, f"{sfx}: {why}"


def test_tree_exact_windows(wa, gpu, monkeypatch, tmp_path):
    """The sorted-exact route (`set_exact_windows`) reaches the kernel: 64 queries with windows of 1 100 .. 2 900 positions that
    all touch position blocks 0 and 1 and no other (every block then has 64 >= 32 wide queries: all are eligible)."""
    sfx, d, n, k, L, nq = "UInt8Euclidian", 1025, 6000, 10, 3000, 64
    rng = np.random.default_rng(8025)
    X, Q = _rows(rng, np.uint8, n, d, "uniform"), _rows(rng, np.uint8, nq, d, "uniform")
    labels = rng.permutation(n).astype(np.float32)
    a = rng.integers(1000, 1901, nq)
    w = np.array([rng.integers(max(1100, BLOCK + 1 - s), min(2900, 2 * BLOCK - s) + 1) for s in a])
    assert ((a < BLOCK) & (a + w > BLOCK) & (a + w <= 2 * BLOCK) & (w >= 1100) & (w <= 2900)).all()
    W = np.stack([a - 0.5, a + w - 0.5], 1).astype(np.float64)
    path = os.path.join(str(tmp_path), "graphs", "")
    os.makedirs(path, exist_ok=True)
    idx = getattr(wa, "VamanaRangeFilterTreeIndex" + sfx)(X, labels, cutoff=500, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, path))
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_DENSE_LONG_ROWS", "1")
    assert idx.set_exact_windows(L) == 0
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    ids0, d0 = idx.batch_search(Q, W, nq, "optimized_postfilter", _qp(wa, k))
    e0 = idx.exact_window_counters()
    assert e0["queries"] == nq and e0["dense_queries"] == 0 and e0["unproven"] == 0 and e0["rescued"] == 0 and e0["passes"] == 0, e0
    monkeypatch.delenv("WANN_NO_GEMM")
    ids1, d1 = idx.batch_search(Q, W, nq, "optimized_postfilter", _qp(wa, k))
    e1 = idx.exact_window_counters()
    _note(f"tree {sfx} d={d} exact windows L={L}: {e1}")
    assert np.array_equal(ids0, ids1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    assert e1["queries"] == nq and e1["dense_queries"] > 0, e1
    # the exact rows: a PrefilterIndex of the same data on its scan
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    pids, pd = pi.batch_search(Q, W, nq, _qp(wa, k))
    ctx = gu.RowContext(X.astype(np.float32), labels, Q.astype(np.float32), W, "l2", "prefilter")
    ok, why = gu.same_rows(pids, pd, ids1, d1, True, ctx)
    assert ok, why


@pytest.mark.parametrize("path", ("shared", "cover"))
def test_long_rows_are_opt_in(wa, gpu, monkeypatch, path):
    """without WANN_DENSE_LONG_ROWS the d = 1025 batch keeps the exact scan: the same rows, every dense counter zero"""
    sfx, d = "UInt8Euclidian", 1025
    bt = _batch(d, _elem(sfx))
    pi = _index(wa, sfx, bt)
    W = bt.windows(path)
    ids1, d1, c1 = _scan_and_dense(pi, wa, monkeypatch, path, bt.Q, W, 10)
    ids0, d0, c0 = _scan_and_dense(pi, wa, monkeypatch, path, bt.Q, W, 10, long_rows=False)
    _note(f"{sfx} d={d} {path} k=10: with the switch {c1}, without {c0}")
    assert c1["queries"] == len(bt.Q), c1
    assert c0 == dict(queries=0, unproven=0, rescued=0), c0
    assert np.array_equal(ids0, ids1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


@pytest.mark.parametrize("sfx", ("UInt8Euclidian", "Int8Mips"))
def test_short_rows_are_untouched_by_the_switch(wa, gpu, monkeypatch, sfx):
    """a d = 512 batch returns the rows and the counters it returns without the switch (guards the dispatch and the key format)"""
    bt = _batch(512, _elem(sfx))
    pi = _index(wa, sfx, bt)
    W = bt.windows("shared")
    ids1, d1, c1 = _scan_and_dense(pi, wa, monkeypatch, "shared", bt.Q, W, 10)
    ids0, d0, c0 = _scan_and_dense(pi, wa, monkeypatch, "shared", bt.Q, W, 10, long_rows=False)
    _note(f"{sfx} d=512 shared k=10: with the switch {c1}, without {c0}")
    assert c1 == c0 and c1["queries"] == len(bt.Q), (c1, c0)
    assert np.array_equal(ids0, ids1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
