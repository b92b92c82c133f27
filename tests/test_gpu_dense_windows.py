"""GPU: distinct wide windows of a PrefilterIndex batch on the matrix cores (cover groups; `set_dense_windows`).

With the option on, the queries that share no window are grouped by 2 048-position block of the label order and scored by the
dense path's kernels; a point of a block that lies outside a query's own window must never come back.  The contract is the
shared-window path's: the rows are the exact scan's -- same index object, option off then on, ids and distance bits equal
row for row -- and whatever the scores cannot settle is counted and handed to the scan."""
import ctypes
import os

import numpy as np
import pytest

import golden_util as gu
from util import mixed_positions as _mixed_positions, pos_windows as _pos_windows, random_rows as _random_rows, repeated_labels

pytestmark = pytest.mark.gpu

MIN_WINDOW, MIN_QUERIES, BLOCK = 1024, 32, 2048  # kCoverMinWindow, kCoverMinQueries, kGemmPointChunk (csrc/wann_gemm_device.h)
ZERO = dict(queries=0, unproven=0, rescued=0, groups=0, tiles=0, passes=0, handover_bytes=0)


def _qp(mod, k=10):
    return mod.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def _elem(sfx):
    return np.uint8 if sfx.startswith("UInt8") else np.int8 if sfx.startswith("Int8") else np.float16 if sfx.startswith("Float16") else np.float32


def _oracle_index(oracle, sfx, X, labels):
    if sfx.startswith("Float16"):
        return getattr(oracle, "PrefilterIndex" + sfx.replace("Float16", "Float"))(X.astype(np.float32), labels), np.float32
    return getattr(oracle, "PrefilterIndex" + sfx)(X, labels), X.dtype


def _eligible(a, b, n, candidates=None):
    """the documented rule: of the candidate queries (those in no shared-window group), the ones whose window holds at least
    MIN_WINDOW positions and touches only blocks that at least MIN_QUERIES such windows touch"""
    wide = (b - a >= MIN_WINDOW) & (np.ones(len(a), dtype=bool) if candidates is None else candidates)
    cover = np.zeros((n - 1) // BLOCK + 2, dtype=np.int64)
    for x, y in zip(a[wide], b[wide]):
        cover[x // BLOCK:(y - 1) // BLOCK + 1] += 1
    return np.array([w and cover[x // BLOCK:(y - 1) // BLOCK + 1].min() >= MIN_QUERIES for x, y, w in zip(a, b, wide)])


def _off_then_on(pi, wa, Q, W, k):
    """the same batch with the option off and on: rows equal bit for bit; returns the rows and both calls' counters"""
    nq = len(Q)
    pi.set_dense_windows(False)
    ids0, d0 = pi.batch_search(Q, W, nq, _qp(wa, k))
    c0 = pi.counters()
    assert pi.dense_window_counters() == ZERO
    assert pi.set_dense_windows(True) is False
    ids1, d1 = pi.batch_search(Q, W, nq, _qp(wa, k))
    c1, w1 = pi.counters(), pi.dense_window_counters()
    assert pi.set_dense_windows(False) is True
    bad = np.nonzero((d0.view(np.uint32) != d1.view(np.uint32)).any(axis=1) | (ids0 != ids1).any(axis=1))[0]
    assert len(bad) == 0, (k, len(bad), bad[:5], ids0[bad[:2]], ids1[bad[:2]], d0[bad[:2]], d1[bad[:2]], w1)
    return ids1, d1, c0, c1, w1


# one row length per class of score kernel: narrow, _wide<2>, _wide4, float16, _b<1..4>, _b<5..8>
EQUAL_CASES = [("FloatEuclidian", 64), ("FloatMips", 100), ("FloatMips", 200), ("FloatEuclidian", 500), ("Float16Euclidian", 100),
               ("Float16Mips", 48), ("UInt8Euclidian", 100), ("UInt8Mips", 400), ("Int8Euclidian", 400), ("Int8Mips", 100)]


@pytest.mark.parametrize("sfx,d", EQUAL_CASES)
def test_cover_path_rows_equal_the_scan(oracle, wa, gpu, monkeypatch, sfx, d):
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    rng = np.random.default_rng(101 + d)
    n, nq = 30000 + 777, 1200
    X, Q = _random_rows(sfx, rng, n, d), _random_rows(sfx, rng, nq, d)
    X[5000:5030] = X[5000]  # duplicates
    labels = rng.permutation(n).astype(np.float32)
    a, b = _mixed_positions(rng, n, nq)
    W = _pos_windows(a, b)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    oi, oq = _oracle_index(oracle, sfx, X, labels)
    ctx = gu.RowContext(X.astype(np.float32), labels, Q.astype(np.float32), W, gu.metric_of(sfx), "prefilter")
    for k in (10, 1, 16):
        ids, dists, c0, c1, w1 = _off_then_on(pi, wa, Q, W, k)
        print(f"[dense windows] {sfx} d={d} k={k}: cover {w1}, brute_rows {c0['brute_rows']} -> {c1['brute_rows']}")
        assert c0["gemm_queries"] == c1["gemm_queries"]
        assert w1["queries"] > nq // 2, w1
        assert c1["brute_rows"] < c0["brute_rows"]
        eids, edists = oi.batch_search(Q.astype(oq), W, nq, _qp(oracle, k))
        ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
        assert ok, f"{sfx} d={d} k={k}: {why}"
        # what the cover path cannot take comes back through the scan with the reference's padding
        assert (ids[50:60] == 0xFFFFFFFF).all() and (ids[40:50, -1] == 0xFFFFFFFF).all() if k > 9 else True


@pytest.mark.parametrize("sfx", ("FloatEuclidian", "FloatMips", "UInt8Euclidian", "Int8Mips", "Float16Mips"))
def test_window_mask(wa, gpu, monkeypatch, sfx):
    """Distinct labels.  Just outside every query's window, at positions a - 1 and b of the label order, lie the best points of
    the whole set for that query (copies of it under L2, a large multiple under the inner product); just inside, at a and b - 1,
    one more copy each.  The outside points never come back; the inside ones are the first two rows."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    rng = np.random.default_rng(7)
    d, k, rep = 64, 10, 40
    slot, nfam = 5000, 40                   # family f owns positions [slot f, slot (f + 1)): planted points never collide
    nq = nfam * rep                         # a family = 40 nested windows [a + 2 j, b - 2 j): every block is covered 40 times
    n = slot * nfam + 500
    X, Q = _random_rows(sfx, rng, n, d), _random_rows(sfx, rng, nq, d)
    if sfx.startswith("Int8"):
        X = (X // 4).astype(np.int8)        # room for a larger multiple of the query
        Q = np.where(Q == 0, 1, Q).astype(np.int8)
    order = rng.permutation(n)              # order[p] = the row at position p of the label order
    labels = np.empty(n, dtype=np.float32)
    labels[order] = np.arange(n, dtype=np.float32)
    fa = slot * np.arange(nfam) + 200 + rng.integers(0, 300, nfam)
    fa[::5] -= fa[::5] % 128                # some edges on step and block boundaries
    fa[2::5] = slot * np.arange(nfam)[2::5] + (BLOCK - (slot * np.arange(nfam)[2::5]) % BLOCK)
    fb = fa + rng.integers(MIN_WINDOW + 250, 2500, nfam)
    fb[1::5] -= fb[1::5] % 64
    j = np.tile(np.arange(rep), nfam)
    a, b = np.repeat(fa, rep) + 2 * j + 1, np.repeat(fb, rep) - 2 * j - 1
    assert (fa > np.concatenate([[0], fb[:-1]])).all() and (b - a >= MIN_WINDOW).all() and fb[-1] < n
    mips = sfx.endswith("Mips")

    def best(q, scale):
        if not mips:
            return q
        if sfx.startswith("Float"):
            # (x 5 outside, x 4 inside: another family member's outside point lies INSIDE the wider windows of its family and
            # must not beat their inside points -- unit vectors of 64 elements stay well below a cosine of 4 / 5)
            return (q.astype(np.float32) * (5 if scale == 8 else 4)).astype(X.dtype)
        return np.clip(q.astype(np.int32) * scale, -128, 127).astype(X.dtype)

    for i in range(nq):  # (positions a - 1, a of the family's windows are all different; so are b - 1, b)
        X[order[a[i] - 1]] = best(Q[i], 8)
        X[order[b[i]]] = best(Q[i], 8)
        X[order[a[i]]] = best(Q[i], 4)
        X[order[b[i] - 1]] = best(Q[i], 4)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    ids, dists, c0, c1, w1 = _off_then_on(pi, wa, Q, _pos_windows(a, b), k)
    print(f"[dense windows] mask {sfx}: {w1}")
    # (where a block boundary falls between a family's outer and inner edges, the block before it is touched by fewer than
    # MIN_QUERIES of its windows, and those few take the scan)
    assert c1["gemm_queries"] == 0 and w1["queries"] >= nq * 9 // 10, (c1, w1)
    for i in range(nq):
        outside = {int(order[a[i] - 1]), int(order[b[i]])}
        assert not (outside & set(ids[i].tolist())), (i, ids[i])
        assert set(ids[i, :2].tolist()) == {int(order[a[i]]), int(order[b[i] - 1])}, (i, ids[i], dists[i])


def _distinct_windows(labels, nq, seed, lo=1100, hi=9000):
    """windows of lo .. hi points with ends from the sorted labels (inside runs of equal labels), no two made alike on purpose"""
    rng = np.random.default_rng(seed)
    s = np.sort(labels)
    n = len(s)
    W = np.zeros((nq, 2))
    for i in range(nq):
        w = int(rng.integers(lo, hi))
        st = int(rng.integers(0, n - w))
        W[i] = (s[st], s[st + w])
    W[-5:] = (s[-3000], s[-1])        # hi = the largest label
    W[-10:-5] = (s[0] - 1, s[2500])   # lo below the smallest label
    return W


@pytest.mark.parametrize("d", (4, 32))
@pytest.mark.parametrize("sfx", ("UInt8Euclidian", "UInt8Mips", "Int8Euclidian", "Int8Mips", "FloatEuclidian", "Float16Mips"))
def test_cover_path_ties(oracle, wa, gpu, monkeypatch, sfx, d):
    """Three-valued elements and repeated labels: most queries have many points at their k-th distance, in and out of what the
    score kernel hands over; rows equal the scan's bit for bit and the oracle's up to its ties."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    rng = np.random.default_rng(41 + d)
    n, nq = 20000, 600
    lo = 0 if sfx.startswith("UInt8") else -1
    X = rng.integers(lo, lo + 3, (n, d)).astype(_elem(sfx))
    Q = rng.integers(lo, lo + 3, (nq, d)).astype(_elem(sfx))
    Q[::4] = X[rng.choice(n, len(Q[::4]))]
    labels = repeated_labels(n, 31, 150)
    W = _distinct_windows(labels, nq, 3)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    oi, oq = _oracle_index(oracle, sfx, X, labels)
    ctx = gu.RowContext(X.astype(np.float32), labels, Q.astype(np.float32), W, gu.metric_of(sfx), "prefilter")
    for k in (10, 1, 16):
        ids, dists, c0, c1, w1 = _off_then_on(pi, wa, Q, W, k)
        print(f"[dense windows] ties {sfx} d={d} k={k}: {w1}")
        assert w1["queries"] > nq // 2, w1
        eids, edists = oi.batch_search(Q.astype(oq), W, nq, _qp(oracle, k))
        ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
        assert ok, f"{sfx} d={d} k={k}: {why}"


@pytest.mark.parametrize("sfx", ("FloatMips", "UInt8Euclidian"))
def test_mixed_batch_uses_both_paths(wa, gpu, monkeypatch, sfx):
    """99 queries on each of a few shared windows plus a few thousand distinct ones: the shared-window groups are what they
    are without the option, the cover path accounts for the rest."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    rng = np.random.default_rng(11)
    n, d, nshared, ndist = 60000, 64, 4, 3000
    X = _random_rows(sfx, rng, n, d)
    labels = rng.permutation(n).astype(np.float32)
    sa = rng.integers(0, n - 12000, nshared)
    a = np.concatenate([np.repeat(sa, 99), rng.integers(0, n - 9000, ndist)])
    b = a + np.concatenate([np.repeat(rng.integers(5000, 12000, nshared), 99), rng.integers(MIN_WINDOW, 9000, ndist)])
    perm = rng.permutation(len(a))
    a, b = a[perm], b[perm]
    Q = _random_rows(sfx, rng, len(a), d)
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    ids, dists, c0, c1, w1 = _off_then_on(pi, wa, Q, _pos_windows(a, b), 10)
    print(f"[dense windows] mixed {sfx}: gemm {c1['gemm_queries']}, cover {w1}")
    assert c0["gemm_queries"] == c1["gemm_queries"] == 99 * nshared, (c0, c1)
    shared = np.isin(a, sa)
    assert shared.sum() == 99 * nshared
    elig = int(_eligible(a, b, n, ~shared).sum())
    assert w1["queries"] == elig and elig > ndist * 9 // 10, (w1, elig)
    assert c1["gemm_unproven"] == c0["gemm_unproven"] and c1["gemm_rescued"] == c0["gemm_rescued"]


USED_CASES = [("FloatEuclidian", 64), ("FloatMips", 128), ("FloatMips", 256), ("Float16Mips", 100), ("UInt8Euclidian", 64),
              ("UInt8Mips", 128), ("Int8Euclidian", 128), ("Int8Mips", 320)]
_observed = []


@pytest.mark.parametrize("sfx,d", USED_CASES)
def test_cover_path_is_really_used(wa, gpu, monkeypatch, sfx, d):
    """Uniform random rows of 64 elements or more, every window above the minimum width and at least 32 queries on every block:
    every query takes the cover path, the scan's rows drop accordingly, and at most a tenth of the queries go back to the scan
    (the cap of the shared-window path on well-spread rows)."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    rng = np.random.default_rng(3 + d)
    n, nq, k = 40000, 2000, 10
    X, Q = _random_rows(sfx, rng, n, d), _random_rows(sfx, rng, nq, d)
    labels = rng.permutation(n).astype(np.float32)
    w = rng.integers(3000, 12000, nq)
    a = (rng.random(nq) * (n - w)).astype(np.int64)
    a[:40], w[:40] = np.arange(40), n - 2 * np.arange(40)  # (both ends of the label order are covered often enough too)
    b = a + w
    cover = np.zeros(n // BLOCK + 2, dtype=np.int64)
    for x, y in zip(a, b):
        cover[x // BLOCK:(y - 1) // BLOCK + 1] += 1
    assert cover[:(n - 1) // BLOCK + 1].min() >= 32
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, labels)
    ids, dists, c0, c1, w1 = _off_then_on(pi, wa, Q, _pos_windows(a, b), k)
    line = f"{sfx} d={d} k={k}: cover queries {w1['queries']} of {nq}, unproven {w1['unproven']}, rescued {w1['rescued']}, " \
           f"groups {w1['groups']}, tiles {w1['tiles']}, passes {w1['passes']}, brute_rows {c0['brute_rows']} -> {c1['brute_rows']}"
    print("[dense windows] used " + line)
    out = os.environ.get("DENSE_WINDOWS_COUNTERS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    assert w1["queries"] == nq, w1
    # (the scan counts the rows of the reference's window rule, which may end a row short of the position range)
    assert abs(c0["brute_rows"] - int(w.sum())) <= nq and c1["gemm_queries"] == 0
    assert w1["unproven"] <= nq // 10, w1
    # the scan only sees what was handed back to it
    assert c1["brute_rows"] <= int(np.sort(w)[nq - w1["unproven"]:].sum()), (c1, w1)


def test_passes_when_the_hand_over_outgrows_the_buffer(wa, gpu, monkeypatch):
    """nq x blocks beyond the score buffer's (query, block) pairs: the batch runs in several passes and no query is left to the
    scan because a buffer was full."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    rng = np.random.default_rng(19)
    n, d, nq = 200_000, 32, 6000      # 98 blocks x 6 000 full-width queries = 588 000 pairs > 524 288
    monkeypatch.delenv("WANN_DENSE_ALWAYS")  # (1.2 G rows of 32 bytes: far above the batch's minimum scan work, no hook needed)
    X = rng.integers(0, 256, (n, d)).astype(np.uint8)
    Q = rng.integers(0, 256, (nq, d)).astype(np.uint8)
    labels = rng.permutation(n).astype(np.float32)
    a = rng.integers(0, 50, nq)
    b = n - rng.integers(0, 50, nq)
    pi = wa.PrefilterIndexUInt8Euclidian(X, labels)
    ids, dists, c0, c1, w1 = _off_then_on(pi, wa, Q, _pos_windows(a, b), 10)
    print(f"[dense windows] passes: {w1}, brute_rows {c0['brute_rows']} -> {c1['brute_rows']}")
    assert w1["queries"] == nq and w1["passes"] >= 2, w1
    assert w1["handover_bytes"] <= w1["passes"] * (256 << 20)


def test_every_call_form(wa, gpu, monkeypatch):
    """device-buffer call with fractional fp32 queries, two asynchronous lanes with different batches in flight, repeated calls
    with alternating batch shapes (workspace reuse), the option toggled between calls"""
    import torch
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    rng = np.random.default_rng(77)
    n, d, k = 50000, 40, 10
    X = rng.integers(0, 256, (n, d)).astype(np.uint8)
    labels = rng.permutation(n).astype(np.float32)
    pi = wa.PrefilterIndexUInt8Euclidian(X, labels)
    dev = torch.device("cuda:0")

    def batch(nq, seed, wmax):
        r = np.random.default_rng(seed)
        Q = (r.random((nq, d)) * 700 - 250).astype(np.float32)  # fractions, negatives, beyond the byte range
        w = r.integers(MIN_WINDOW, wmax, nq)
        a = (r.random(nq) * (n - w)).astype(np.int64)
        return torch.from_numpy(Q).to(dev), torch.from_numpy(_pos_windows(a, a + w).astype(np.float32)).to(dev), nq

    def run(bt, on):
        tq, tw, nq = bt
        pi.set_dense_windows(on)
        ti = torch.zeros((nq, k), dtype=torch.int32, device=dev)
        td = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        pi.batch_search_device(tq.data_ptr(), tw.data_ptr(), nq, 0, "", _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0)
        return ti.cpu().numpy(), td.cpu().numpy(), pi.dense_window_counters()

    shapes = [batch(1500, 1, 9000), batch(300, 2, 30000), batch(4000, 3, 5000), batch(64, 4, 50000 - 1)]
    want = [run(bt, False) for bt in shapes]
    assert all(w[2] == ZERO for w in want)
    for rnd in range(2):
        for bt, w in zip(shapes, want):  # alternating shapes, option on; then toggled off and on again
            got = run(bt, True)
            assert got[2]["queries"] > 0 or bt[2] < 300, got[2]
            assert np.array_equal(got[0], w[0]) and np.array_equal(got[1].view(np.uint32), w[1].view(np.uint32))
            off = run(bt, False)
            assert off[2] == ZERO and np.array_equal(off[0], w[0])
    # two lanes, two different batches in flight
    pi.set_dense_windows(True)
    outs, tickets = [], []
    for bt in (shapes[0], shapes[2]):
        tq, tw, nq = bt
        ti = torch.zeros((nq, k), dtype=torch.int32, device=dev)
        td = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        outs.append((ti, td))
        torch.cuda.synchronize()
        tickets.append(pi.batch_search_device_async(tq.data_ptr(), tw.data_ptr(), nq, 0, "", _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0))
    for t in tickets:
        pi.wait(t)
    for (ti, td), w in zip(outs, (want[0], want[2])):
        assert np.array_equal(ti.cpu().numpy(), w[0]) and np.array_equal(td.cpu().numpy().view(np.uint32), w[1].view(np.uint32))
    assert pi.dense_window_counters()["queries"] > 0


def test_no_gemm_hook_turns_the_cover_path_off(wa, gpu, monkeypatch):
    rng = np.random.default_rng(5)
    n, d, nq = 30000, 32, 500
    X, Q = _random_rows("Int8", rng, n, d), _random_rows("Int8", rng, nq, d)
    labels = rng.permutation(n).astype(np.float32)
    a = rng.integers(0, n - 8000, nq)
    b = a + rng.integers(2000, 8000, nq)
    W = _pos_windows(a, b)
    pi = wa.PrefilterIndexInt8Mips(X, labels)
    pi.set_dense_windows(True)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    r0 = pi.batch_search(Q, W, nq, _qp(wa))
    assert pi.dense_window_counters() == ZERO
    monkeypatch.delenv("WANN_NO_GEMM")
    r1 = pi.batch_search(Q, W, nq, _qp(wa))
    assert pi.dense_window_counters()["queries"] == int(_eligible(a, b, n).sum()) > nq * 9 // 10
    assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1].view(np.uint32), r1[1].view(np.uint32))


def test_small_batches_keep_the_scan(wa, gpu, monkeypatch):
    """the measured crossover: a batch whose eligible windows hold less than 2 GiB of rows in all is faster on the scan, and the
    option leaves it there (the hook WANN_DENSE_ALWAYS, which the other tests of this file set, lifts the minimum)"""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.delenv("WANN_DENSE_ALWAYS", raising=False)
    rng = np.random.default_rng(5)
    n, d, nq = 30000, 32, 500
    X, Q = _random_rows("Float", rng, n, d), _random_rows("Float", rng, nq, d)
    labels = rng.permutation(n).astype(np.float32)
    a = rng.integers(0, n - 8000, nq)
    b = a + rng.integers(2000, 8000, nq)
    assert int((b - a).sum()) * d * 4 < 2 ** 31
    pi = wa.PrefilterIndexFloatEuclidian(X, labels)
    pi.set_dense_windows(True)
    r0 = pi.batch_search(Q, _pos_windows(a, b), nq, _qp(wa))
    assert pi.dense_window_counters() == ZERO and pi.counters()["brute_rows"] > 0
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    r1 = pi.batch_search(Q, _pos_windows(a, b), nq, _qp(wa))
    assert pi.dense_window_counters()["queries"] == int(_eligible(a, b, n).sum()) > 0
    assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1].view(np.uint32), r1[1].view(np.uint32))


def test_off_means_off(wa, gpu, monkeypatch):
    """the option never set: a wide-window batch leaves the cover counters at zero"""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    rng = np.random.default_rng(5)
    n, d, nq = 30000, 32, 500
    X, Q = _random_rows("Float", rng, n, d), _random_rows("Float", rng, nq, d)
    labels = rng.permutation(n).astype(np.float32)
    a = rng.integers(0, n - 8000, nq)
    b = a + rng.integers(2000, 8000, nq)
    pi = wa.PrefilterIndexFloatEuclidian(X, labels)
    pi.batch_search(Q, _pos_windows(a, b), nq, _qp(wa))
    assert pi.dense_window_counters() == ZERO
    c = pi.counters()
    assert c["gemm_queries"] == 0 and c["brute_rows"] == int((b - a).sum())
    assert not hasattr(wa.RangeFilterTreeIndexFloatEuclidian, "set_dense_windows")  # (PrefilterIndex classes only)


class _Counters(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in ("queries", "unproven", "rescued", "groups", "tiles", "passes", "handover_bytes")]


def test_through_the_c_abi(wa, gpu, monkeypatch):
    """wann_set_dense_windows / wann_get_dense_window_counters through ctypes: previous setting returned, other kinds refused
    with a negative code, rows equal with the option off and on"""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work, see test_small_batches_keep_the_scan)
    import rangefilteredann_amd
    lib = ctypes.CDLL(os.path.join(os.path.dirname(rangefilteredann_amd.__file__), "libwann.so"))
    lib.wann_index_create.restype = ctypes.c_void_p
    lib.wann_index_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.wann_index_destroy.argtypes = [ctypes.c_void_p]
    lib.wann_set_dense_windows.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.wann_get_dense_window_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Counters)]
    lib.wann_batch_search.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_char_p] + [ctypes.c_void_p] * 3
    assert lib.wann_abi_version() == 5

    class QP(ctypes.Structure):
        _fields_ = [("k", ctypes.c_int64), ("beam_width", ctypes.c_int64), ("cut", ctypes.c_double), ("limit", ctypes.c_int64),
                    ("degree_limit", ctypes.c_int64), ("final_beam_multiply", ctypes.c_int64), ("postfiltering_max_beam", ctypes.c_int64),
                    ("has_ratio", ctypes.c_int32), ("ratio", ctypes.c_float), ("verbose", ctypes.c_int32)]

    rng = np.random.default_rng(2)
    n, d, nq, k = 30000, 64, 800, 10
    X = np.ascontiguousarray(_random_rows("Float", rng, n, d))
    Q = np.ascontiguousarray(_random_rows("Float", rng, nq, d))
    labels = rng.permutation(n).astype(np.float32)
    a = rng.integers(0, n - 8000, nq)
    b = a + rng.integers(2000, 8000, nq)
    elig = int(_eligible(a, b, n).sum())
    assert elig > nq * 9 // 10
    W = np.ascontiguousarray(_pos_windows(a, b).astype(np.float32))
    h = lib.wann_index_create(0, 1, 0, X.ctypes.data, n, d, labels.ctypes.data, 1000, 2.0, 0.5, None, 0, 4)
    assert h
    qp = QP(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, 0, 0.0, 0)
    rows = []
    try:
        for on in (0, 1):
            assert lib.wann_set_dense_windows(h, on) == 0
            ids = np.zeros((nq, k), dtype=np.uint32)
            dists = np.zeros((nq, k), dtype=np.float32)
            assert lib.wann_batch_search(h, Q.ctypes.data, W.ctypes.data, nq, b"", ctypes.byref(qp), ids.ctypes.data, dists.ctypes.data) == 0
            c = _Counters()
            assert lib.wann_get_dense_window_counters(h, ctypes.byref(c)) == 0
            assert c.queries == (elig if on else 0) and (c.passes == 1 if on else c.handover_bytes == 0)
            rows.append((ids, dists))
        assert lib.wann_set_dense_windows(h, 0) == 1
        assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1].view(np.uint32), rows[1][1].view(np.uint32))
    finally:
        lib.wann_index_destroy(h)
    small, small_labels = np.ascontiguousarray(X[:3000]), np.ascontiguousarray(labels[:3000])
    t = lib.wann_index_create(2, 1, 0, small.ctypes.data, 3000, d, small_labels.ctypes.data, 1000, 2.0, 0.5, None, 0, 4)
    assert t
    try:
        assert lib.wann_set_dense_windows(t, 1) == -5 and lib.wann_set_dense_windows(t, 0) == 0
    finally:
        lib.wann_index_destroy(t)
