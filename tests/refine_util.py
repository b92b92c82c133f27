"""The refined search (include/wann.h REFINED SEARCH) restated in numpy, for the tests: what
wann_batch_search_device_refined must return, given what the ordinary call returned at k = refine_k.  Distances come from the
oracle's distance() -- the float32 index's arithmetic and evaluation order -- so ids AND distance bits can be compared."""
import ctypes

import numpy as np

FLT_MAX = np.float32(3.402823466e+38)
PAD_SORTED, PAD_RAW = 0, 0xFFFFFFFF  # padding ids: the sorted kinds (tree classes) / the post filter and the PrefilterIndex


def pad_id_of(kind):
    return PAD_SORTED if kind.endswith("TreeIndex") else PAD_RAW


def fkey(dist):
    """the kernels' order-preserving float32 -> uint32 map (wann_wave.h fkey): ascending keys = ascending distances, -0.0 before +0.0"""
    u = np.asarray(dist, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def candidate_counts(ids, dists, pad_id):
    """entries of each row before its first pad (id == pad_id and dist == FLT_MAX)"""
    pad = (np.asarray(ids).astype(np.uint32) == np.uint32(pad_id)) & (np.asarray(dists, dtype=np.float32) == FLT_MAX)
    return np.where(pad.any(axis=1), pad.argmax(axis=1), pad.shape[1])


def refine_reference(oracle, metric, rows32, Q, ids, dists, k, pad_id):
    """ids / dists: the ordinary call's rows at k = refine_k, (nq, refine_k).  Returns (ids, dists) of shape (nq, k): per query
    the candidates -- the entries before the first pad -- scored as (rows32[id], Q[q]) by oracle.distance, the first k under
    (refined distance, id), then pads (pad_id, FLT_MAX).  Duplicate ids stay duplicate."""
    rows32 = np.ascontiguousarray(rows32, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    ids = np.asarray(ids).astype(np.uint32)
    nq, d = ids.shape[0], rows32.shape[1]
    cnt = candidate_counts(ids, dists, pad_id)
    out_i = np.full((nq, k), pad_id, dtype=np.uint32)
    out_d = np.full((nq, k), FLT_MAX, dtype=np.float32)
    dist = oracle.lib().orc_distance
    for q in range(nq):
        c = ids[q, :cnt[q]].astype(np.int64)
        if not len(c):
            continue
        qp = Q[q].ctypes.data_as(ctypes.c_void_p)
        rd = np.array([dist(metric, rows32[i].ctypes.data_as(ctypes.c_void_p), qp, d) for i in c], dtype=np.float32)
        order = np.lexsort((c, fkey(rd)))[:k]
        out_i[q, :len(order)] = c[order]
        out_d[q, :len(order)] = rd[order]
    return out_i, out_d


def self_test(oracle):
    """refine_reference on hand-made rows (no GPU): pads in the middle of a batch, an all-pad row, duplicate ids, equal refined
    distances broken by id, k == refine_k"""
    rows = np.array([[0, 0], [1, 0], [0, 1], [3, 0], [0, 3], [2, 2], [1, 0], [5, 5]], dtype=np.float32)  # rows 1 and 6 are equal
    Q = np.zeros((5, 2), dtype=np.float32)
    P = PAD_RAW
    big = FLT_MAX
    ids = np.array([[7, 3, 1, 0],          # full row: re-ordered by the refined distance
                    [5, P, P, P],          # pads after one candidate
                    [P, P, P, P],          # all pads
                    [6, 2, 1, 6],          # a duplicate id, and three rows at distance 1: (1, id 1), (1, id 2), (1, id 6), (1, id 6)
                    [4, 3, P, P]], dtype=np.uint32)
    dists = np.array([[9, 9, 9, 9], [9, big, big, big], [big] * 4, [9, 9, 9, 9], [9, 9, big, big]], dtype=np.float32)
    gi, gd = refine_reference(oracle, oracle.L2, rows, Q, ids, dists, 2, P)
    assert gi.tolist() == [[0, 1], [5, P], [P, P], [1, 2], [3, 4]], gi
    assert gd.tolist() == [[0, 1], [8, big], [big, big], [1, 1], [9, 9]], gd
    # k == refine_k: every candidate comes back, duplicates included, pads stay a suffix
    gi, gd = refine_reference(oracle, oracle.L2, rows, Q, ids, dists, 4, P)
    assert gi.tolist() == [[0, 1, 3, 7], [5, P, P, P], [P] * 4, [1, 2, 6, 6], [3, 4, P, P]], gi
    assert gd[3].tolist() == [1, 1, 1, 1] and gd[0].tolist() == [0, 1, 9, 50]
    assert candidate_counts(ids, dists, P).tolist() == [4, 1, 0, 4, 2]
    # a pad is BOTH fields: id 0 at FLT_MAX is a candidate of a raw-id kind, and the padding of a sorted kind
    one = (np.array([[0, 0]], dtype=np.uint32), np.array([[big, big]], dtype=np.float32))
    assert candidate_counts(*one, PAD_RAW).tolist() == [2] and candidate_counts(*one, PAD_SORTED).tolist() == [0]
    # the inner product: the distance is minus the product, ties by id
    gi, gd = refine_reference(oracle, oracle.MIPS, rows, np.array([[1, 1]], dtype=np.float32), np.array([[2, 1, 7, 0]], dtype=np.uint32),
                              np.zeros((1, 4), dtype=np.float32), 3, P)
    assert gi.tolist() == [[7, 1, 2]] and gd.tolist() == [[-10, -1, -1]]
    assert fkey(np.float32(-0.0)) < fkey(np.float32(0.0)) < fkey(np.float32(1e-45)) and fkey(np.float32(-1)) < fkey(np.float32(-0.0))
