"""Shared helpers for the test-suite: seeded synthetic inputs shaped like the reference's datasets
 and stdout silencing for the chatty reference module."""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


@contextlib.contextmanager
def quiet_stdout():
    """Silence C++ std::cout of the reference module (build timers, cache messages)."""
    sys.stdout.flush()
    saved = os.dup(1)
    devnull = os.open(os.devnull, os.O_WRONLY)
    os.dup2(devnull, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)
        os.close(devnull)


def sift_like(n, d, seed, latent=16):
    """Integer-valued floats in [0,255] with low intrinsic dimension: fp32 sums are exact in any order."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((latent, d))

    def gen(m):
        z = rng.standard_normal((m, latent))
        x = z @ A * 18 + 128 + rng.standard_normal((m, d)) * 6
        return np.clip(np.rint(x), 0, 255).astype(np.float32)

    return gen


def unit_mixture(n, d, seed, latent=24, clusters=50):
    """Unit-norm rows of a Gaussian mixture (GloVe/deep-like, used with MIPS)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((latent, d)) / np.sqrt(latent)
    cent = rng.standard_normal((clusters, latent)) * 1.5

    def gen(m):
        c = rng.integers(0, clusters, m)
        z = cent[c] + rng.standard_normal((m, latent))
        x = z @ A + 0.1 * rng.standard_normal((m, d))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return x.astype(np.float32)

    return gen


def distinct_labels(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.permutation(n) + 0.5) / n).astype(np.float32)


def windows(labels, nq, p, seed):
    """nq label windows covering a 2^p fraction of the points (generate_datasets/filter_generation_utils.py:9-74,
    simplified: start uniform, [s[start], s[start+w]]; p = 0 -> everything)."""
    rng = np.random.default_rng(seed)
    n = len(labels)
    s = np.sort(labels)
    w = max(1, int(n * 2.0 ** p))
    out = np.zeros((nq, 2), dtype=np.float64)
    for i in range(nq):
        if w >= n - 2:
            out[i] = (s[0] - 1, s[-1] + 1)
        else:
            st = int(rng.integers(1, n - w - 1))
            out[i] = (s[st], s[st + w])
    return out


def brute_force_gt(X, labels, Q, W, k, metric):
    """Exact filtered top-k ids (float64 arithmetic)."""
    out = []
    Xd = X.astype(np.float64)
    for q, (lo, hi) in zip(Q.astype(np.float64), W):
        idx = np.nonzero((labels >= np.float32(lo)) & (labels <= np.float32(hi)))[0]
        if metric == "mips":
            dist = -(Xd[idx] @ q)
        else:
            dist = ((Xd[idx] - q) ** 2).sum(axis=1)
        out.append(idx[np.argsort(dist, kind="stable")[:k]])
    return out


def recall(gt, ids, k=10):
    """mean |gt ∩ res[:k]| / |gt|  (experiments/run_our_method.py:174-180)"""
    tot = 0.0
    cnt = 0
    for g, r in zip(gt, ids):
        if len(g) == 0:
            continue
        tot += len(set(g.tolist()) & set(r[:k].tolist())) / len(g)
        cnt += 1
    return tot / max(cnt, 1)


def clustered_window_batch(d, style, seed=17, nclu=12, per=1500, qper=40):
    """The batch of the dense prefilter tests, shaped like generate_datasets/generate_advserial_dataset.py:8-69: nclu clusters of
    `per` points whose labels are c - 0.5 + U(0, 1), and qper queries per cluster that share the cluster's window; every seventh
    query takes a second shared window and a few get a window of their own.  style "sift": integer-valued rows in [0, 255]
    (sift_like); "unit": cluster centres plus noise, float64 and NOT normalised -- a caller normalises and quantises row by row.
    Returns X (rows shuffled), Q, labels, W."""
    rng = np.random.default_rng(seed)
    n = nclu * per
    if style == "sift":
        X, Q = sift_like(n, d, 3)(n), sift_like(n, d, 3)(nclu * qper)
    else:
        cent = rng.standard_normal((nclu, d))
        X = cent[np.repeat(np.arange(nclu), per)] + 0.3 * rng.standard_normal((n, d))
        Q = cent[np.repeat(np.arange(nclu), qper)] + 0.3 * rng.standard_normal((nclu * qper, d))
    labels = (np.repeat(np.arange(nclu), per) - 0.5 + rng.random(n)).astype(np.float32)
    perm = rng.permutation(n)
    X, labels = X[perm], labels[perm]
    W = np.zeros((Q.shape[0], 2))
    cl = np.repeat(np.arange(nclu), qper)
    W[:, 0], W[:, 1] = cl - 0.5, cl + 0.5
    W[::7] = (2.2, 3.9)       # a second family of shared windows
    W[5::31, 1] += 1e-3 * np.arange(len(W[5::31]))  # and some unique ones (exact scan)
    return X, Q, labels, W


def tie_heavy(n, d, seed, lo=0, hi=12, dup_frac=0.15, zero_rows=0):
    """Rows of small integers in [lo, hi) as float32 (exact in fp32, bf16, uint8 / int8): nearly every distance is shared by many
    points.  A dup_frac share of the rows copies other rows, and a block of zero_rows rows in the middle is all zero."""
    rng = np.random.default_rng(seed)
    X = rng.integers(lo, hi, size=(n, d)).astype(np.float32)
    ndup = int(n * dup_frac)
    X[rng.choice(n, ndup, replace=False)] = X[rng.choice(n, ndup)]
    if zero_rows:
        at = (n - zero_rows) // 2
        X[at:at + zero_rows] = 0
    return X


def tie_queries(X, nq, seed, lo=0, hi=12):
    """Queries over the same small integers: a quarter of them are points of X, and the last one is all zero."""
    rng = np.random.default_rng(seed)
    Q = rng.integers(lo, hi, size=(nq, X.shape[1])).astype(np.float32)
    Q[::4] = X[rng.choice(len(X), len(Q[::4]))]
    Q[-1] = 0
    return Q


def star_hub(n, d, metric, hub_ids, norms=(8.0,), seed=0, elem=None):
    """Points of which nearly every one chooses the same out-neighbour (a HUB), so that a whole insertion batch of the graph
    builder becomes one reverse-edge group for that node.  hub_ids: the rows that become hubs -- a hub collects (nearly) every
    row of a partition only when it is the partition's start point, start + oracle.random_permutation(size)[0].
    metric "mips": rows with positive coordinates on the unit sphere; hub j is norms[j] times a unit vector with equal
    coordinates, over all d dimensions when there is one hub, over the j-th of len(hub_ids) equal slices of the dimensions
    otherwise (hubs orthogonal to each other: one hub does not prune another out of a row, every hub prunes ordinary points).
    metric "l2": standard-normal rows scaled to unit length (mixed signs), the (single) hub is the zero vector.
    elem = np.uint8 (mips): integers 0 .. 15, the hub row is all 255.  Returns float32 rows, or rows of `elem`."""
    rng = np.random.default_rng(seed)
    hub_ids = [int(h) for h in hub_ids]
    norms = list(norms) + [norms[-1]] * (len(hub_ids) - len(norms))
    if elem is not None:
        assert metric == "mips" and len(hub_ids) == 1
        X = rng.integers(0, 16, size=(n, d)).astype(elem)
        X[hub_ids[0]] = 255
        return X
    X = rng.standard_normal((n, d))
    if metric == "mips":
        X = np.abs(X)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    if metric == "mips":
        w = d // len(hub_ids)
        for j, h in enumerate(hub_ids):
            X[h] = 0
            lo, hi = (0, d) if len(hub_ids) == 1 else (j * w, (j + 1) * w)
            X[h, lo:hi] = norms[j] / np.sqrt(hi - lo)
    else:
        assert len(hub_ids) == 1
        X[hub_ids[0]] = 0
    return X.astype(np.float32)


def tree_hub_ids(oracle, n):
    """star_hub's hub_ids for a tree with split_factor 2 over ascending labels (ids are positions): the start points of the
    root partition and of its two halves"""
    half = n // 2
    c = int(oracle.random_permutation(half)[0])
    return [int(oracle.random_permutation(n)[0]), c, half + c]


def repeated_labels(n, seed, n_values):
    """Labels drawn from n_values distinct float32 values: runs of about n / n_values points share a label."""
    rng = np.random.default_rng(seed)
    return ((rng.integers(0, n_values, n) + 1.0) / n_values).astype(np.float32)


def tie_windows(labels, nq, p, seed):
    """windows() of a 2^p fraction, and where labels repeat, every fifth row of each of the windows that end inside runs:
    [v, v] (zero width, a whole run carries v), [v1, v2] with both ends existing labels, hi equal to the largest label,
    lo below the smallest label."""
    out = windows(labels, nq, p, seed)
    s = np.sort(labels)
    if len(np.unique(s)) == len(s):
        return out
    rng = np.random.default_rng(seed + 1)
    n = len(s)
    w = max(1, int(n * 2.0 ** p))
    for i in range(nq):
        st = int(rng.integers(0, n - w))
        kind = i % 5
        if kind == 1:
            out[i] = (s[st], s[st])
        elif kind == 2:
            out[i] = (s[st], s[st + w])
        elif kind == 3:
            out[i] = (s[n - 1 - w], s[-1])
        elif kind == 4:
            out[i] = (s[0] - 1, s[w])
    return out


# ---- inputs shared by the dense-window, exact-window and result-width GPU tests ---------------------------------------------
COVER_MIN_WINDOW, GEMM_POINT_CHUNK = 1024, 2048  # kCoverMinWindow, kGemmPointChunk (csrc/wann_gemm_device.h)


def elem_type(sfx):
    """numpy element type of the index class whose name ends in sfx ("UInt8Euclidian", "Float16Mips", "Float", ...)"""
    return np.uint8 if sfx.startswith("UInt8") else np.int8 if sfx.startswith("Int8") else np.float16 if sfx.startswith("Float16") else np.float32


def random_rows(sfx, rng, n, d):
    """well-spread rows: uniform random bytes, unit vectors for the float types"""
    if sfx.startswith("UInt8"):
        return rng.integers(0, 256, (n, d)).astype(np.uint8)
    if sfx.startswith("Int8"):
        return rng.integers(-128, 128, (n, d)).astype(np.int8)
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(elem_type(sfx))


def pos_windows(a, b):
    """label windows that hold exactly positions [a, b) of the label order when labels are a permutation of 0 .. n-1"""
    return np.stack([np.asarray(a, dtype=np.float64) - 0.5, np.asarray(b, dtype=np.float64) - 0.5], 1)


def mixed_positions(rng, n, nq):
    """window positions [a, b): several fractions of n, edges on and off multiples of 64, 128 and 2 048, the whole set, windows
    below the minimum width, empty ones, ones with fewer than 16 points and ones outside the label span"""
    a = np.zeros(nq, dtype=np.int64)
    b = np.zeros(nq, dtype=np.int64)
    for i in range(nq):
        w = int(n * (1 / 32, 1 / 8, 1 / 2, 1 / 16)[i % 4] * (0.6 + 0.8 * rng.random()))
        w = max(w, COVER_MIN_WINDOW + 1)
        st = int(rng.integers(0, n - w))
        kind = i % 7
        if kind == 1:
            st -= st % 64
        elif kind == 2:
            st -= st % 128
            w -= w % 128
        elif kind == 3:
            st -= st % GEMM_POINT_CHUNK
            w = max(GEMM_POINT_CHUNK, w - w % GEMM_POINT_CHUNK)
        elif kind == 4:
            e = (st + w) - (st + w) % GEMM_POINT_CHUNK
            w = e - st if e - st >= COVER_MIN_WINDOW else w
        a[i], b[i] = st, min(n, st + w)
    a[0], b[0] = 0, n                       # the whole set
    a[1], b[1] = 0, n
    a[10:40] = rng.integers(0, n - 1000, 30)
    b[10:40] = a[10:40] + rng.integers(17, COVER_MIN_WINDOW, 30)    # below the minimum width
    b[40:50] = a[40:50] + rng.integers(1, 10, 10)              # fewer than k points
    b[50:55] = a[50:55]                                        # empty
    a[55:60], b[55:60] = n + 100, n + 5000                     # beyond the label span
    a[60:62], b[60:62] = n - 1500, n                           # up to the last point
    return a, b


def wide_window_batch(n, nq, seed):
    """nq windows of 3 000 .. 12 000 positions (start a, width w) that cover every 2 048-point block of the label order at least
    32 times, both ends included"""
    rng = np.random.default_rng(seed)
    w = rng.integers(3000, 12000, nq)
    a = (rng.random(nq) * (n - w - 2)).astype(np.int64) + 1
    # (both ends of the label order are covered often enough too)
    a[:40], w[:40] = 1 + np.arange(40), 11000 - 2 * np.arange(40)
    w[40:80] = 11000 - 2 * np.arange(40)
    a[40:80] = n - 1 - w[40:80] - np.arange(40)
    cover = np.zeros(n // GEMM_POINT_CHUNK + 2, dtype=np.int64)
    for x, y in zip(a, a + w):
        cover[x // GEMM_POINT_CHUNK:(y - 1) // GEMM_POINT_CHUNK + 1] += 1
    assert cover[:(n - 1) // GEMM_POINT_CHUNK + 1].min() >= 32
    return a, w
