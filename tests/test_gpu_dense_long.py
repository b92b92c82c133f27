"""GPU: float32 rows of 513 .. 2048 elements on the dense paths (`k_gemm_scores_long`).

The score kernel walks such a row in a run-time number of 128-float slabs (the last one shorter, in multiples of 16), both
operands staged per slab.  The row lengths here are the slab counts and last-slab shapes at which such a loop goes wrong; n is
the smallest at which a window spans two position blocks and ends in a ragged step.  Per case:
  1. under WANN_NO_GEMM the batch runs on the exact scan alone (dense counters zero);
  2. the dense path's rows are the scan's, ids and distance bits, row for row (k_rerank's keys are the scan's);
  3. the scan's rows are the oracle's PrefilterIndex rows (distances bit for bit, ids up to exact ties);
  4. every eligible query is counted on its path (zero for these lengths before the kernel existed);
  5. at most a tenth of the batch is unproven on these well-spread rows -- a kernel that settles nothing would otherwise pass on
     the scan's rows.
Counters are printed per case and appended to $DENSE_LONG_COUNTERS_OUT when set."""
import os

import numpy as np
import pytest

import golden_util as gu
import numerics_util as nu

pytestmark = pytest.mark.gpu

ZERO = dict(queries=0, unproven=0, rescued=0, groups=0, tiles=0, passes=0, handover_bytes=0)
EXACT_ZERO = dict(queries=0, dense_queries=0, unproven=0, rescued=0, passes=0, rows_scanned=0)
BLOCK = nu.BLOCK
N = 3 * BLOCK + 64
F, REP = 6, nu.REP
# 513 pads to 528: four full slabs and one of 16 floats; 640: exactly five; 768: six; 1000 pads to 1008: a last slab of 112;
# 1536: twelve; 2048: the limit
DIMS = (513, 640, 768, 1000, 1536, 2048)
SFX = ("FloatEuclidian", "FloatMips")


def _qp(mod, k=10):
    return mod.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def _note(line):
    print("[dense long] " + line)
    out = os.environ.get("DENSE_LONG_COUNTERS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


class _Batch:
    """N unit-norm Gaussian rows with distinct labels in a random order, and F families of REP queries.  Family f shares the
    window [a_f, b_f) of 1 700 .. 3 000 positions (even f: a_f a multiple of 128, odd f: not); on the cover path query j of the
    family has [a_f + j, b_f - j).  The ends are drawn so that all REP windows of a family touch the same position blocks: every
    block a query touches then has at least REP >= 32 wide queries, and every query is eligible for the cover path.  No window
    reaches the last 64 positions (the reference's scan never returns the last point)."""

    def __init__(self, d):
        rng = np.random.default_rng(7000 + d)
        self.d = d
        self.X = _unit(rng.standard_normal((N, d)))
        self.Q = _unit(rng.standard_normal((F * REP, d)))
        self.order = rng.permutation(N)
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


_batches, _indexes = {}, {}


def _batch(d):
    if d not in _batches:
        _batches.clear()  # (one row length at a time: 50 MB at d = 2048)
        _indexes.clear()
        _batches[d] = _Batch(d)
    return _batches[d]


def _index(wa, sfx, bt):
    if (sfx, bt.d) not in _indexes:
        _indexes[sfx, bt.d] = getattr(wa, "PrefilterIndex" + sfx)(bt.X, bt.labels)
    return _indexes[sfx, bt.d]


def _scan_and_dense(pi, wa, monkeypatch, path, Q, W, k):
    """the batch on the exact scan (dense counters zero), then on the dense path `path`: rows equal bit for bit.  Returns the
    scan's rows and the path's counters."""
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work for the cover path)
    monkeypatch.setenv("WANN_DENSE_LONG_ROWS", "1")  # (rows of more than 512 floats take the dense path where the process opts in)
    nq = len(Q)
    pi.set_dense_windows(False)
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    ids0, d0 = pi.batch_search(Q, W, nq, _qp(wa, k))
    assert pi.counters()["gemm_queries"] == 0 and pi.dense_window_counters() == ZERO
    monkeypatch.delenv("WANN_NO_GEMM")
    pi.set_dense_windows(path == "cover")
    ids1, d1 = pi.batch_search(Q, W, nq, _qp(wa, k))
    c, w = pi.counters(), pi.dense_window_counters()
    pi.set_dense_windows(False)
    if path == "cover":
        assert c["gemm_queries"] == 0, c
        ctr = dict(queries=w["queries"], unproven=w["unproven"], rescued=w["rescued"])
    else:
        assert w == ZERO, w
        ctr = dict(queries=c["gemm_queries"], unproven=c["gemm_unproven"], rescued=c["gemm_rescued"])
    bad = np.nonzero((d0.view(np.uint32) != d1.view(np.uint32)).any(axis=1) | (ids0 != ids1).any(axis=1))[0]
    assert len(bad) == 0, (path, k, len(bad), bad[:5], ids0[bad[:2]], ids1[bad[:2]], d0[bad[:2]], d1[bad[:2]], ctr)
    return ids0, d0, ctr


def _case(oracle, wa, monkeypatch, sfx, d, path, k):
    bt = _batch(d)
    pi = _index(wa, sfx, bt)
    W = bt.windows(path)
    ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, path, bt.Q, W, k)
    eids, edists = bt.oracle_rows(oracle, sfx, path, k)
    ctx = gu.RowContext(bt.X, bt.labels, bt.Q, W, gu.metric_of(sfx), "prefilter")
    ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
    assert ok, f"{sfx} d={d} {path} k={k}: {why}"
    _note(f"{sfx} d={d} {path} k={k}: {ctr}")
    assert ctr["queries"] == len(bt.Q), (sfx, d, path, ctr)  # every query of these batches is eligible for its path
    assert ctr["unproven"] <= len(bt.Q) // 10, (sfx, d, path, ctr)


SHARED_CASES = [(d, k) for d in DIMS for k in ((10, 1, 16) if d == 768 else (10,))]


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d,k", SHARED_CASES)
def test_shared_windows(oracle, wa, gpu, monkeypatch, sfx, d, k):
    _case(oracle, wa, monkeypatch, sfx, d, "shared", k)


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d", (513, 1000, 2048))
def test_cover_groups(oracle, wa, gpu, monkeypatch, sfx, d):
    _case(oracle, wa, monkeypatch, sfx, d, "cover", 10)


def test_tree_exact_windows(wa, gpu, monkeypatch, tmp_path):
    """The sorted-exact route (`set_exact_windows`) reaches the kernel: 64 queries with windows of 1 100 .. 2 900 positions that
    all touch position blocks 0 and 1 and no other (every block then has 64 >= 32 wide queries: all are eligible)."""
    sfx, d, n, k, L, nq = "FloatEuclidian", 768, 6000, 10, 3000, 64
    rng = np.random.default_rng(7768)
    X, Q = _unit(rng.standard_normal((n, d))), _unit(rng.standard_normal((nq, d)))
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
    assert e1["queries"] == nq and e1["dense_queries"] == nq, e1
    assert e1["unproven"] <= nq // 10, e1
    # the exact rows: a PrefilterIndex of the same data on its scan
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    pids, pd = pi.batch_search(Q, W, nq, _qp(wa, k))
    ok, why = gu.same_rows(pids, pd, ids1, d1, True, gu.RowContext(X, labels, Q, W, "l2", "prefilter"))
    assert ok, why


@pytest.mark.parametrize("path", ("shared", "cover"))
def test_near_ties(oracle, wa, gpu, monkeypatch, path):
    """d = 768, L2: shells of 128 points whose exact distances differ by about 2^-21 relative (numerics_util.Families), scattered
    over the window and contiguous.  Rows equal the scan's; over the shell queries unproven + rescued is at least the number of
    queries for which the score model says the top 10 is not within the 32 best scores; the control queries keep the cap."""
    sfx, d, k = "FloatEuclidian", 768, 10
    fam = nu.Families(5000 + d, d, ["scattered", "contiguous", "control"] * 2)
    pi = getattr(wa, "PrefilterIndex" + sfx)(fam.X, fam.labels)
    shell, control = np.nonzero(fam.is_shell)[0], np.nonzero(~fam.is_shell)[0]
    W = fam.windows(path)
    ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, path, fam.Q, W, k)
    assert ctr["queries"] == len(fam.Q), ctr
    oi = getattr(oracle, "PrefilterIndex" + sfx)(fam.X, fam.labels)
    eids, edists = oi.batch_search(fam.Q, W, len(fam.Q), _qp(oracle, k))
    ok, why = gu.same_rows(eids, edists, ids, dists, True, gu.RowContext(fam.X, fam.labels, fam.Q, W, "l2", "prefilter"))
    assert ok, why
    need = int(fam.outside_keep("l2", k)[shell].sum())
    _, _, cs = _scan_and_dense(pi, wa, monkeypatch, path, np.ascontiguousarray(fam.Q[shell]), W[shell], k)
    _, _, cc = _scan_and_dense(pi, wa, monkeypatch, path, np.ascontiguousarray(fam.Q[control]), W[control], k)
    _note(f"near ties {sfx} d={d} {path} k={k}: batch {ctr}; shell queries {cs}, model says {need} of {len(shell)} cannot be settled; "
          f"control queries {cc}")
    assert cs["queries"] == len(shell) and cc["queries"] == len(control), (cs, cc)
    assert cs["unproven"] + cs["rescued"] >= need, (cs, need)
    assert cc["unproven"] <= len(control) // 10, cc


@pytest.mark.parametrize("path", ("shared", "cover"))
@pytest.mark.parametrize("sfx", SFX)
def test_beyond_the_limit(oracle, wa, gpu, monkeypatch, sfx, path):
    """d = 2049 (rows padded to 2064 floats): the exact scan answers, no dense counter moves, no error"""
    bt = _batch(2049)
    pi = _index(wa, sfx, bt)
    W = bt.windows(path)
    ids, dists, ctr = _scan_and_dense(pi, wa, monkeypatch, path, bt.Q, W, 10)
    assert ctr == dict(queries=0, unproven=0, rescued=0), ctr
    eids, edists = bt.oracle_rows(oracle, sfx, path, 10)
    ok, why = gu.same_rows(eids, edists, ids, dists, True, gu.RowContext(bt.X, bt.labels, bt.Q, W, gu.metric_of(sfx), "prefilter"))
    assert ok, why
    _note(f"{sfx} d=2049 {path} k=10: {ctr}")


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d", (128, 512))
def test_existing_lengths_keep_their_kernels(oracle, wa, gpu, monkeypatch, sfx, d):
    """rows of up to 512 floats report the counters they reported before the long-row kernel (guards the dispatch)"""
    _case(oracle, wa, monkeypatch, sfx, d, "shared", 10)
