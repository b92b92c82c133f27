"""The wide call (include/wann.h WIDE ROWS) restated on the CPU oracle, for the tests: what
wann_batch_search_device_wide must return.  The oracle itself needs no change: ONE oracle call with
QueryParams(k=W, beam_width=b, final_beam_multiply=1, postfiltering_max_beam=b+1) runs exactly one level of the doubling loop
at beam b (the level finds fewer than W entries -> the beam doubles to 2 b >= b + 1 and the loop ends; W entries -> it ends
at once; the final re-search is min(b * 1, b + 1) = b: none) and returns that level's first W in-window entries.  restate()
composes such calls into the loop of postfilter_vamana.h:161-181 with knn = s, per query.

A level call is always made on the WHOLE batch -- a query's row number is its own id in the search (beamSearch.h:128) -- and
the rows of the queries that are at that level are taken from it.  Queries whose window is answered by an exact scan (tiny
windows of the tree classes) get the same row from every level call: the best W of the window.

The cases of the issue that introduced the call are here too, so that the CPU test of the restatement and the GPU tests of
the engine run the same inputs."""
import numpy as np

import refine_util as ru

N, D, NQ = 3000, 20, 200
R, L, ALPHA, CUTOFF = 16, 40, 1.2, 300
WIDTHS = (0.02, 0.05, 0.1, 0.3)
# (s, W, B, final_beam_multiply, postfiltering_max_beam): s = the stop threshold, W = the row width, B = the first beam
PARAMS = ((5, 20, 8, 1, 10000), (10, 40, 16, 2, 10000), (3, 64, 4, 1, 100))
# (class name without element type and metric, method): the three kinds with a graph search
KINDS = (("PostfilterVamanaIndex", ""), ("VamanaRangeFilterTreeIndex", "optimized_postfilter"), ("SuperOptimizedPostfilterTreeIndex", ""))
# the nine cases the restatement was first run on (the oracle alone: 68 - 200 of the 200 rows held more than s entries, 94 - 200
# differed from the ordinary call at k = W)
RECORDED = (("PostfilterVamanaIndex", "Euclidian"), ("VamanaRangeFilterTreeIndex", "Euclidian"), ("SuperOptimizedPostfilterTreeIndex", "Mips"))


def data(seed=1, n=N, d=D, nq=NQ):
    """standard-normal points and queries, uniform labels (float32, distinct for these seeds), windows of WIDTHS[i % 4]"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    labels = rng.random(n).astype(np.float32)
    w = np.array([WIDTHS[i % len(WIDTHS)] for i in range(nq)])
    lo = rng.random(nq) * (1 - w)
    return X, Q, labels, np.stack([lo, lo + w], 1)


def kwargs_of(mod, kind, cache, cutoff=CUTOFF):
    kw = dict(build_params=mod.BuildParams(R, L, ALPHA, cache))
    if kind != "PostfilterVamanaIndex":
        kw.update(cutoff=cutoff, split_factor=2)
    if kind == "SuperOptimizedPostfilterTreeIndex":
        kw.update(shift_factor=0.5)
    return kw


def qp(mod, k, beam, mult, max_beam):
    return mod.QueryParams(k, beam, 1.35, 10_000_000, 10_000, mult, max_beam, None, False)


def search(idx, Q, W, nq, method, params):
    return idx.batch_search(Q, W, nq, method, params) if method else idx.batch_search(Q, W, nq, params)


def restate(orc, idx, Q, W, nq, method, s, width, B, mult, max_beam, pad_id):
    """rows (nq, width) of the wide call at (stop_k = s, width) on the oracle index idx; also returns the number of level calls"""
    cache = {}

    def level(b):
        if b not in cache:
            ids, dists = search(idx, Q, W, nq, method, qp(orc, width, b, 1, b + 1))
            cache[b] = (ids, dists, ru.candidate_counts(ids, dists, pad_id))
        return cache[b]

    out_i = np.full((nq, width), pad_id, dtype=np.uint32)
    out_d = np.full((nq, width), ru.FLT_MAX, dtype=np.float32)
    for q in range(nq):
        b, res = B, None
        while (res is None or res[2][q] < s) and b < max_beam:  # postfilter_vamana.h:161-172
            res = level(b)
            if res[2][q] < s:
                b *= 2
        fb = min(b * mult, max_beam)  # :173-181
        if fb > b:
            res = level(fb)
        if res is not None:
            out_i[q], out_d[q] = res[0][q], res[1][q]
    return (out_i, out_d), len(cache)
