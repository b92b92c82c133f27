"""The register-resident small-beam core (beams <= 128) on rows built to reach every branch of its seen-filter's class loop
and of its two union loops: `wa.raw_beam_search` against `oracle.beam_search` -- ids, distance bits, sizes, hops, dist_cmps.

The filter has 2^bits slots, bits = oracle.hash_bits(beam).  Two lanes of a row that share a slot form a clashing class; a
node listed twice sits inside one class, and only such a row sends the union down the general multiset loop -- every other
row, clashing or not, takes the lean loop.  Rows are edited after the build, per filter size, to begin with one of
  (a) three ids of one slot                      (b) two clashing classes
  (c) (x, y, x), y in x's slot: both copies pass the filter and the multiset rule keeps two
  (d) (x, x): the second copy is dropped by the filter
  (e) (x, y, x, z, x), y and z in x's slot
  (f) two different ids of one slot and a duplicate-free tail: a clash without a duplicate (lean loop after the class loop)
The start node's row carries several (c) triples whose x are nearest neighbours of queries, so that at every beam some
query's final beam holds an id twice.  That, and that some query visits a row of every kind, is checked on the oracle alone
(test_rows_reach_every_case needs no GPU)."""
import functools

import numpy as np
import pytest

from util import sift_like, unit_mixture

N, NQ, R, L_BUILD, START, SN = 6000, 64, 64, 100, 300, 5000
CASES = {0: (sift_like, 128), 1: (unit_mixture, 100)}
BEAMS = (16, 40, 64, 65, 80, 100, 128)  # NE = 1: 2^10 slots; NE = 2: 2^11, 2^11, 2^12, 2^12 slots
KINDS = "abcdef"
PER_KIND = 60


def _orc():
    from oracle import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=None)
def _data(metric):
    orc = _orc()
    gen, d = CASES[metric]
    g = gen(N, d, 12)
    X, Q = g(N), g(NQ)
    Xp = orc.pad_rows(X)
    rows = orc.vamana_build(Xp, d, metric, START, SN, R, L_BUILD, 1.2)
    P, Qd = X[START:START + SN].astype(np.float64), Q.astype(np.float64)
    score = -(Qd @ P.T) if metric == 1 else (P * P).sum(1)[None, :] - 2.0 * (Qd @ P.T)  # (the order per query is all that is used)
    near = np.argsort(score, axis=1, kind="stable")[:, :3]  # the three nearest nodes of every query, partition-local ids
    qids = np.arange(NQ, dtype=np.int64) + 10**6
    return X, Q, Xp, d, rows, near, qids


def _pattern(kind, x, grp, other):
    """the row prefix of a kind: x's slot holds grp (x first), `other` is a class of another slot"""
    if kind == "a":
        return [grp[0], grp[1], grp[2]]
    if kind == "b":
        return [grp[0], other[0], grp[1], other[1]]
    if kind == "c":
        return [x, grp[1], x]
    if kind == "d":
        return [x, x]
    if kind == "e":
        return [x, grp[1], x, grp[2], x]
    return [grp[0], grp[1]]


@functools.lru_cache(maxsize=None)
def _edited_rows(metric, bits):
    """(rows, {kind: set of rows}) for the filter of 2^bits slots"""
    orc = _orc()
    X, Q, Xp, d, rows0, near, qids = _data(metric)
    rows = rows0.copy()
    mask = (1 << bits) - 1
    slot = np.array([orc.hash64_2(i) & mask for i in range(SN)])
    members = {}
    for i, s in enumerate(slot):
        members.setdefault(int(s), []).append(i)
    trio = [i for i in range(SN) if len(members[int(slot[i])]) >= 3]  # ids with two or more companions in their slot
    assert len(trio) > 100, (bits, len(trio))

    def group(x):  # x and then its slot's other ids
        return [x] + [i for i in members[int(slot[x])] if i != x]

    def put(r, pat):
        tail = [int(t) for t in rows[r, 1:1 + rows[r, 0]] if int(t) not in pat]
        lst = (pat + tail)[:R]
        rows[r, 0] = len(lst)
        rows[r, 1:1 + len(lst)] = lst
        rows[r, 1 + len(lst):] = 0

    rng = np.random.default_rng(1000 * metric + bits)
    by_kind = {k: set() for k in KINDS}
    chosen = rng.choice(np.arange(1, SN), PER_KIND * len(KINDS), replace=False)
    for n_, r in enumerate(chosen):
        kind = KINDS[n_ % len(KINDS)]
        x = int(trio[int(rng.integers(len(trio)))])
        y = int(trio[int(rng.integers(len(trio)))])
        while slot[y] == slot[x]:
            y = int(trio[int(rng.integers(len(trio)))])
        put(int(r), _pattern(kind, x, group(x), group(y)))
        by_kind[kind].add(int(r))
    # the start node's row: (c) triples around nearest neighbours of queries, each in a slot of its own
    pat, used = [], set()
    for x in (int(v) for v in near.ravel()):
        if len(members[int(slot[x])]) >= 2 and int(slot[x]) not in used and x != 0:
            used.add(int(slot[x]))
            pat += [x, group(x)[1], x]
        if len(used) == 12:
            break
    put(0, pat)
    by_kind["c"].add(0)
    by_kind["b"].add(0)
    return rows, by_kind


@functools.lru_cache(maxsize=None)
def _expected(metric, beam):
    orc = _orc()
    X, Q, Xp, d, _, _, qids = _data(metric)
    rows, _ = _edited_rows(metric, orc.hash_bits(beam))
    return [orc.beam_search(rows, Xp, d, metric, START, Q[i], int(qids[i]), beam) for i in range(NQ)]


def _check_conditions(metric, beam):
    orc = _orc()
    _, by_kind = _edited_rows(metric, orc.hash_bits(beam))
    exp = _expected(metric, beam)
    assert any(len(set(oi.tolist())) < len(oi) for oi, *_ in exp), ("no beam holds an id twice", metric, beam)
    for kind in KINDS:
        assert any(by_kind[kind] & set(vi.tolist()) for _, _, vi, _, _ in exp), ("no query visits a row of kind", kind, metric, beam)


def test_filter_sizes_are_the_kernels():
    """bits = max(10, ceil(log2(beam^2)) - 2), as hash_bits_dev in the search kernels"""
    assert [_orc().hash_bits(b) for b in BEAMS] == [max(10, (b * b - 1).bit_length() - 2) for b in BEAMS] == [10, 10, 10, 11, 11, 12, 12]


@pytest.mark.parametrize("beam", BEAMS)
@pytest.mark.parametrize("metric", [0, 1])
def test_rows_reach_every_case(metric, beam):
    """the oracle alone: some final beam holds an id twice, and rows of every kind are visited"""
    _check_conditions(metric, beam)


@pytest.mark.gpu
@pytest.mark.parametrize("beam", BEAMS)
@pytest.mark.parametrize("metric", [0, 1])
def test_small_core_union_matches_oracle(oracle, wa, gpu, metric, beam):
    _check_conditions(metric, beam)
    X, Q, Xp, d, _, _, qids = _data(metric)
    rows, _ = _edited_rows(metric, oracle.hash_bits(beam))
    ids, dists, sizes, hops, cmps = wa.raw_beam_search(metric, X, rows, START, Q, qids, beam)
    for i, (oi, od, vi, vd, dc) in enumerate(_expected(metric, beam)):
        m = int(sizes[i])
        assert m == len(oi), (beam, i, m, len(oi))
        assert np.array_equal(ids[i, :m], oi), (beam, i)
        assert np.array_equal(dists[i, :m].view(np.uint32), od.view(np.uint32)), (beam, i)
        assert int(hops[i]) == len(vi) and int(cmps[i]) == dc, (beam, i, hops[i], len(vi), cmps[i], dc)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [0, 1])
def test_small_core_union_on_tie_heavy_data(oracle, wa, gpu, metric):
    """Small integer coordinates and duplicate rows (the recipe of test_raw_beam_search_on_tie_heavy_data) on R = 64 graphs:
    candidates of one hop share distances, so the lean loop's key order rests on the ids alone, and a candidate whose distance
    equals the beam's last entry's is common."""
    n, nq, d = 4000, 48, 6
    rng = np.random.default_rng(99)
    X = rng.integers(0, 12, size=(n, d)).astype(np.float32)
    X[rng.choice(n, 600, replace=False)] = X[rng.choice(n, 600)]  # duplicate rows
    Q = rng.integers(0, 12, size=(nq, d)).astype(np.float32)
    Q[::4] = X[rng.choice(n, len(Q[::4]))]                        # queries that ARE points
    Xp = oracle.pad_rows(X)
    start, sn = 200, 3600
    rows = oracle.vamana_build(Xp, d, metric, start, sn, R, 2 * R, 1.0)
    qids = np.arange(nq, dtype=np.int64) + 10**6
    bad = []
    for beam in (20, 64, 100, 128):
        ids, dists, sizes, hops, cmps = wa.raw_beam_search(metric, X, rows, start, Q, qids, beam)
        for i in range(nq):
            oi, od, vi, vd, dc = oracle.beam_search(rows, Xp, d, metric, start, Q[i], int(qids[i]), beam)
            m = int(sizes[i])
            if not (m == len(oi) and np.array_equal(ids[i, :m], oi) and np.array_equal(dists[i, :m].view(np.uint32), od.view(np.uint32))
                    and int(hops[i]) == len(vi) and int(cmps[i]) == dc):
                bad.append((beam, i, m, len(oi), int(hops[i]), len(vi), int(cmps[i]), dc))
    assert not bad, (len(bad), bad[:10])
