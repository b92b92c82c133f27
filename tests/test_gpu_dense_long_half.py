"""GPU: float16 rows of 129 .. 2048 elements on the dense paths (`k_gemm_scores_hslab`).

The score kernel is the float32 K-loop (`k_gemm_scores_long`) with half loads: a run-time number of 128-element slabs, the last
one shorter, both operands staged per slab.  A row of halves is padded to a multiple of 32 while the query operand and the
k-steps go by d rounded up to 16, so the row lengths here are the slab counts, last-slab shapes and paddings at which such a loop
goes wrong; n is the smallest at which a window spans two position blocks and ends in a ragged step.  The rows are those of the
float32 test (tests/test_gpu_dense_long.py) rounded to float16.  Per case, where the process opts in (WANN_DENSE_LONG_ROWS=1):
  1. under WANN_NO_GEMM the batch runs on the exact scan alone (dense counters zero);
  2. the dense path's rows are the scan's, ids and distance bits, row for row;
  3. the scan's rows are the float32 oracle's PrefilterIndex rows on the exact upcast (distances bit for bit, ids up to ties);
  4. every eligible query is counted on its path (zero for these lengths before the kernel existed);
  5. at most a tenth of the batch is unproven on these well-spread rows -- a kernel that settles nothing would otherwise pass on
     the scan's rows;
  6. the float32 index on the upcast rows returns the same rows, and from 513 elements on (where it runs the same K-loop) the
     same counters: the staged operands are the same bits.
Counters are printed per case and appended to $DENSE_LONG_HALF_COUNTERS_OUT when set.

No near-tie case: numerics_util.Families in its grid mode keeps the shells' 2^-21 spread off the grid, so its shell rows are not
halves (rounded, each shell collapses to one point and the score model has nothing left that cannot be settled)."""
import os

import numpy as np
import pytest

import dense_long_half_inputs as inp
import golden_util as gu

pytestmark = pytest.mark.gpu

ZERO = dict(queries=0, unproven=0, rescued=0, groups=0, tiles=0, passes=0, handover_bytes=0)
BLOCK, SFX = inp.BLOCK, inp.SFX
_unit16, _f32, _qp = inp.unit16, inp.f32_class, inp.qp


def _note(line):
    print("[dense long half] " + line)
    out = os.environ.get("DENSE_LONG_HALF_COUNTERS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


_batches, _indexes = {}, {}


def _batch(d):
    if d not in _batches:
        _batches.clear()  # (one row length at a time)
        _indexes.clear()
        _batches[d] = inp.Batch(d)
    return _batches[d]


def _index(wa, sfx, bt):
    """the index of class suffix sfx on the batch's rows: a float16 class on the halves, a float32 class on their upcast"""
    if (sfx, bt.d) not in _indexes:
        _indexes[sfx, bt.d] = getattr(wa, "PrefilterIndex" + sfx)(bt.X if "Float16" in sfx else bt.X32, bt.labels)
    return _indexes[sfx, bt.d]


def _dense(pi, wa, path, Q, W, k):
    """the batch on the dense path `path` (the switches are the caller's): rows and the path's counters"""
    pi.set_dense_windows(path == "cover")
    ids, dists = pi.batch_search(Q, W, len(Q), _qp(wa, k))
    c, w = pi.counters(), pi.dense_window_counters()
    pi.set_dense_windows(False)
    if path == "cover":
        assert c["gemm_queries"] == 0, c
        ctr = dict(queries=w["queries"], unproven=w["unproven"], rescued=w["rescued"])
    else:
        assert w == ZERO, w
        ctr = dict(queries=c["gemm_queries"], unproven=c["gemm_unproven"], rescued=c["gemm_rescued"])
    return ids, dists, ctr


def _scan_and_dense(pi, wa, monkeypatch, path, Q, W, k, long_rows=True):
    """the batch on the exact scan (dense counters zero), then on the dense path `path`: rows equal bit for bit.  Returns the
    scan's rows and the path's counters."""
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work for the cover path)
    if long_rows:
        monkeypatch.setenv("WANN_DENSE_LONG_ROWS", "1")  # (rows of more than 128 halves take the dense path where the process opts in)
    else:
        monkeypatch.delenv("WANN_DENSE_LONG_ROWS", raising=False)
    pi.set_dense_windows(False)
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    ids0, d0 = pi.batch_search(Q, W, len(Q), _qp(wa, k))
    assert pi.counters()["gemm_queries"] == 0 and pi.dense_window_counters() == ZERO
    monkeypatch.delenv("WANN_NO_GEMM")
    ids1, d1, ctr = _dense(pi, wa, path, Q, W, k)
    bad = np.nonzero((d0.view(np.uint32) != d1.view(np.uint32)).any(axis=1) | (ids0 != ids1).any(axis=1))[0]
    assert len(bad) == 0, (path, k, len(bad), bad[:5], ids0[bad[:2]], ids1[bad[:2]], d0[bad[:2]], d1[bad[:2]], ctr)
    return ids0, d0, ctr


def _oracle_check(oracle, bt, sfx, path, k, ids, dists):
    eids, edists = bt.oracle_rows(oracle, sfx, path, k)
    ctx = gu.RowContext(bt.X32, bt.labels, bt.Q32, bt.windows(path), gu.metric_of(sfx), "prefilter")
    ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
    assert ok, f"{sfx} d={bt.d} {path} k={k}: {why}"


def _case(oracle, wa, monkeypatch, sfx, d, path, k):
    bt = _batch(d)
    W = bt.windows(path)
    ids, dists, ctr = _scan_and_dense(_index(wa, sfx, bt), wa, monkeypatch, path, bt.Q, W, k)
    _oracle_check(oracle, bt, sfx, path, k, ids, dists)
    # the float32 index on the upcast rows, on its own dense path (d <= 512: the register-operand kernels, d >= 513: the K-loop)
    fids, fdists, fctr = _dense(_index(wa, _f32(sfx), bt), wa, path, bt.Q32, W, k)
    _note(f"{sfx} d={d} {path} k={k}: {ctr}; float32 index on the upcast: {fctr}")
    assert ctr["queries"] == len(bt.Q), (sfx, d, path, ctr)  # every query of these batches is eligible for its path
    assert ctr["unproven"] <= len(bt.Q) // 10, (sfx, d, path, ctr)
    assert np.array_equal(fids, ids) and np.array_equal(fdists.view(np.uint32), dists.view(np.uint32)), (sfx, d, path, k)
    if d >= 513:
        assert fctr == ctr, (sfx, d, path, ctr, fctr)  # the same arithmetic on the same bits


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d,k", inp.SHARED_CASES)
def test_shared_windows(oracle, wa, gpu, monkeypatch, sfx, d, k):
    _case(oracle, wa, monkeypatch, sfx, d, "shared", k)


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("d", inp.COVER_DIMS)
def test_cover_groups(oracle, wa, gpu, monkeypatch, sfx, d):
    _case(oracle, wa, monkeypatch, sfx, d, "cover", 10)


@pytest.mark.parametrize("path", ("shared", "cover"))
@pytest.mark.parametrize("sfx", SFX)
def test_beyond_the_limit(oracle, wa, gpu, monkeypatch, sfx, path):
    """d = 2049 (2064 floats of the upcast): the exact scan answers, no dense counter moves, no error"""
    bt = _batch(2049)
    ids, dists, ctr = _scan_and_dense(_index(wa, sfx, bt), wa, monkeypatch, path, bt.Q, bt.windows(path), 10)
    assert ctr == dict(queries=0, unproven=0, rescued=0), ctr
    _oracle_check(oracle, bt, sfx, path, 10, ids, dists)
    _note(f"{sfx} d=2049 {path} k=10: {ctr}")


@pytest.mark.parametrize("path", ("shared", "cover"))
@pytest.mark.parametrize("sfx", SFX)
def test_without_the_switch(oracle, wa, gpu, monkeypatch, sfx, path):
    """d = 256 in a process that does not opt in: the rows are the scan's and the oracle's, every dense counter stays zero"""
    bt = _batch(256)
    ids, dists, ctr = _scan_and_dense(_index(wa, sfx, bt), wa, monkeypatch, path, bt.Q, bt.windows(path), 10, long_rows=False)
    assert ctr == dict(queries=0, unproven=0, rescued=0), ctr
    _oracle_check(oracle, bt, sfx, path, 10, ids, dists)
    _note(f"{sfx} d=256 {path} k=10 without WANN_DENSE_LONG_ROWS: {ctr}")


@pytest.mark.parametrize("long_rows", (True, False))
@pytest.mark.parametrize("sfx", SFX)
def test_existing_length_keeps_its_kernel(oracle, wa, gpu, monkeypatch, sfx, long_rows):
    """rows of 100 elements take the narrow kernel, with or without the switch (guards the dispatch)"""
    bt = _batch(100)
    ids, dists, ctr = _scan_and_dense(_index(wa, sfx, bt), wa, monkeypatch, "shared", bt.Q, bt.windows("shared"), 10, long_rows=long_rows)
    _oracle_check(oracle, bt, sfx, "shared", 10, ids, dists)
    _note(f"{sfx} d=100 shared k=10 switch={long_rows}: {ctr}")
    assert ctr["queries"] == len(bt.Q), ctr


def test_tree_exact_windows(wa, gpu, monkeypatch, tmp_path):
    """The sorted-exact route (`set_exact_windows`) reaches the kernel: 64 queries with windows of 1 100 .. 2 900 positions that
    all touch position blocks 0 and 1 and no other (every block then has 64 >= 32 wide queries: all are eligible)."""
    sfx, d, n, k, L, nq = "Float16Euclidian", 768, 6000, 10, 3000, 64
    rng = np.random.default_rng(7768)
    X, Q = _unit16(rng.standard_normal((n, d))), _unit16(rng.standard_normal((nq, d)))
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
    ok, why = gu.same_rows(pids, pd, ids1, d1, True, gu.RowContext(X.astype(np.float32), labels, Q.astype(np.float32), W, "l2", "prefilter"))
    assert ok, why
