"""Input of tests/test_gpu_dense_window_edges.py: windows placed on the edges of the sparse table of `window_norm_max`.

One point set of unit-norm Gaussian rows and queries (numerics_util.Families' control kind) under a random label permutation.
The label order holds disjoint SITES: site s is one window [lo, hi) with REP queries, covered by the 64-position blocks b0 .. b1,
m = b1 - b0 + 1 of them, and separated from its neighbours' blocks by at least three whole blocks.  The block counts reach the
table's levels 4 .. 8 at 2^j, 2^j + 1 and 2^(j+1) - 1; the offsets of lo and hi - 1 inside their blocks are written out below.  n
is 37 past a multiple of 64 (a partial last block) and the last site ends at hi = n - 1, inside that block.

A PLACEMENT names positions, at every site, whose rows a test scales to a huge norm: inside the window where the lookup's two
runs start, end, meet or do not overlap, or just outside the covering blocks."""
import numpy as np

import numerics_util as nu

BLOCK = 64  # kNormBlock
REP = nu.REP
MIN_WINDOW = 1024  # kGroupMinWindow, kCoverMinWindow
GROUP_MIN_QUERIES = 16  # kGroupMinQueries: that many queries of one window are a shared-window group, on either path
# (blocks, lo % 64, (hi - 1) % 64, the ends the cover path's queries shrink: l, h), in label order.  The 16-block site is exactly
# 1 024 positions, both ends on a block boundary: no second window of the minimum width has its blocks, so it has no cover form.
# The last site's (hi - 1) % 64 is what n - 1 makes it: 35.
SITES = [(16, 0, 63, ""), (33, 12, 45, "lh"), (64, 0, 50, "lh"), (17, 3, 60, "h"), (257, 9, 47, "lh"), (65, 17, 62, "lh"),
         (32, 7, 63, "lh"), (127, 1, 41, "h"), (63, 24, 39, "lh"), (129, 21, 35, "l")]
GAPS = (3, 5, 7)  # whole blocks between two sites' covers, in turn
FIRST_BLOCK = 6
IN_WINDOW = ("first", "last", "run_end", "second_only", "first_only")
PLACEMENTS = IN_WINDOW + ("outside", "clean")


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


class Sites:
    """tail_share = (num, den): floor(n num / den) more rows at the END of the label order, at least 256 positions after the last
    window, for the caller to scale (tail_pos); n is then what that comes to, and the last site no longer ends at the table's"""

    def __init__(self, seed, d, tail_share=None):
        rng = np.random.default_rng(seed)
        self.d, self.S = d, len(SITES)
        self.m, self.b0, self.b1, self.lo, self.hi, self.shrink = [], [], [], [], [], []
        b = FIRST_BLOCK
        for s, (m, lo_off, hi_off, ends) in enumerate(SITES):
            self.m.append(m), self.b0.append(b), self.b1.append(b + m - 1), self.shrink.append(ends)
            self.lo.append(BLOCK * b + lo_off), self.hi.append(BLOCK * (b + m - 1) + hi_off + 1)
            b += m + GAPS[s % len(GAPS)]
        self.m, self.b0, self.b1, self.lo, self.hi = (np.array(v, dtype=np.int64) for v in (self.m, self.b0, self.b1, self.lo, self.hi))
        self.n_sites = n0 = int(self.hi[-1]) + 1  # (position n - 1 is in no window: the reference's scan never returns the last point)
        assert n0 % BLOCK == 37 and self.b1[-1] == (n0 - 1) // BLOCK and (self.lo[1:] - self.hi[:-1] >= 3 * BLOCK).all()
        self.tail_pos = np.zeros(0, dtype=np.int64)
        self.n = n0
        if tail_share is not None:  # t = floor(n * num / den) rows after a gap of at least 256 positions
            num, den = tail_share
            n = ((n0 + 256) * den + den - num - 1) // (den - num)
            while n - n * num // den < n0 + 256:
                n += 1
            self.n = n
            self.tail_pos = np.arange(n - n * num // den, n)
            assert len(self.tail_pos) == n * num // den and self.tail_pos[0] - self.hi.max() >= 256
        n = self.n
        self.X = _unit(rng.standard_normal((n, d))).astype(np.float32)
        self.Q = _unit(rng.standard_normal((self.S * REP, d))).astype(np.float32)
        self.order = rng.permutation(n)  # order[p] = the row at position p of the label order
        self.labels = np.empty(n, dtype=np.float32)
        self.labels[self.order] = np.arange(n, dtype=np.float32)
        self.site_of = np.repeat(np.arange(self.S), REP)
        for pl in PLACEMENTS:
            for path in ("shared", "cover"):
                self.positions(path, pl)  # (the assertions in there)

    def level(self, s):
        return int(self.m[s]).bit_length() - 1  # floor(log2 m): the level the lookup reads

    def outliers(self, placement):
        """{site: positions} -- the sites the placement applies to"""
        out = {}
        for s in range(self.S):
            lo, hi, b0, b1, run = int(self.lo[s]), int(self.hi[s]), int(self.b0[s]), int(self.b1[s]), 1 << self.level(s)
            more = int(self.m[s]) > run  # (the two runs are not the same run)
            if placement == "first":
                pos = [lo]
            elif placement == "last":
                pos = [hi - 1]
            elif placement == "run_end":  # the last position of the first run (m = 2^j and hi off the boundary: past the window)
                pos = [BLOCK * (b0 + run - 1) + BLOCK - 1]
                pos = pos if pos[0] < hi else []
            elif placement == "second_only":  # the first block that only the second run covers
                pos = [BLOCK * (b0 + run)] if more else []
            elif placement == "first_only":  # the last block that only the first run covers
                pos = [BLOCK * (b1 - run) + BLOCK - 1] if more else []
            elif placement == "outside":  # one position before and one after the covering blocks
                pos = [p for p in (BLOCK * b0 - 1, BLOCK * (b1 + 1)) if p < self.n]
            else:
                assert placement == "clean"
                pos = []
            if pos:
                out[s] = pos
        return out

    def all_outliers(self, placement):
        return np.array(sorted(p for v in self.outliers(placement).values() for p in v), dtype=np.int64)

    def sites_of(self, path, placement="clean"):
        """the sites a test of this path and placement looks at"""
        have = self.outliers(placement) if placement in IN_WINDOW else {s: [] for s in range(self.S)}
        return [s for s in sorted(have) if path == "shared" or self.shrink[s]]

    def positions(self, path, placement="clean"):
        """[a, b) of every query, as positions.  shared: the site's window.  cover: query i of a site has the window shrunk by i
        positions at the ends the site declares -- but never past the placement's outlier, and never out of the end's block;
        where that leaves no declared end, at the other one, by as much as there is room for."""
        a, b = self.lo[self.site_of].copy(), self.hi[self.site_of].copy()
        inside = self.outliers(placement) if placement in IN_WINDOW else {}
        every = self.all_outliers(placement)
        i = np.arange(REP)
        for s in range(self.S):
            lo, hi, q = int(self.lo[s]), int(self.hi[s]), slice(s * REP, (s + 1) * REP)
            if path == "cover" and self.shrink[s]:
                pos = inside.get(s, [])
                room = {"l": min([REP - 1, BLOCK - 1 - lo % BLOCK] + [p - lo for p in pos]),
                        "h": min([REP - 1, (hi - 1) % BLOCK] + [hi - 1 - p for p in pos])}
                ends = [e for e in self.shrink[s] if room[e] == REP - 1] or [max("lh", key=lambda e: room[e])]
                if "l" in ends:
                    a[q] += i % (room["l"] + 1)
                if "h" in ends:
                    b[q] -= i % (room["h"] + 1)
                _, alike = np.unique(np.stack([a[q], b[q]], 1), axis=0, return_counts=True)
                assert alike.max() < GROUP_MIN_QUERIES, (s, placement, alike)  # (no shared-window group forms)
            # the same blocks for every query of the site; every outlier of the placement in or out of all of them as declared
            assert (a[q] // BLOCK == self.b0[s]).all() and ((b[q] - 1) // BLOCK == self.b1[s]).all(), (s, path, placement)
            assert (b[q] - a[q] >= MIN_WINDOW).all() and (a[q] >= lo).all() and (b[q] <= hi).all(), (s, path, placement)
            for p in every:
                want = p in inside.get(s, [])
                assert (((a[q] <= p) & (p < b[q])) == want).all(), (s, path, placement, p)
                assert want or not self.b0[s] <= p // BLOCK <= self.b1[s], (s, placement, p)  # (the others: outside the cover)
        assert not ((a <= self.n - 1) & (self.n - 1 < b)).any()
        for p in self.tail_pos[:1]:
            assert p - b.max() >= 256
        return a, b

    def queries(self, sites):
        return np.concatenate([np.arange(s * REP, (s + 1) * REP) for s in sites])
