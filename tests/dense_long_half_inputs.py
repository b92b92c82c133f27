"""Inputs of the float16 long-row dense tests: the batches tests/test_gpu_dense_long_half.py runs on the device and
tests/test_dense_long_half_api.py models on the CPU -- the rows of the float32 test (tests/test_gpu_dense_long.py, the same seeds)
rounded to float16."""
import numpy as np

import numerics_util as nu

BLOCK = nu.BLOCK
N = 3 * BLOCK + 64
F, REP = 6, nu.REP
# 129: qw 144 but 160 halves a row (one full slab + 16, the two paddings differ); 160: qw = halves a row; 256: exactly two slabs;
# 500: qw 512, four; 513: qw 528; 768: six; 1000: qw 1008, a last slab of 112; 2048: the limit
DIMS = (129, 160, 256, 500, 513, 768, 1000, 2048)
SFX = ("Float16Euclidian", "Float16Mips")
SHARED_CASES = [(d, k) for d in DIMS for k in ((10, 1, 16) if d == 768 else (10,))]
COVER_DIMS = (129, 1000, 2048)


def qp(mod, k=10):
    return mod.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def unit16(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32).astype(np.float16)


def f32_class(sfx):
    return sfx.replace("Float16", "Float")


class Batch:
    """N unit-norm Gaussian rows rounded to float16, distinct labels in a random order, and F families of REP queries (rounded as
    well: a float16 index takes its queries as halves).  Family f shares the window [a_f, b_f) of 1 700 .. 3 000 positions (even
    f: a_f a multiple of 128, odd f: not); on the cover path query j of the family has [a_f + j, b_f - j).  The ends are drawn so
    that all REP windows of a family touch the same position blocks: every block a query touches then has at least REP >= 32 wide
    queries, and every query is eligible for the cover path.  No window reaches the last 64 positions (the reference's scan never
    returns the last point)."""

    def __init__(self, d):
        rng = np.random.default_rng(7000 + d)
        self.d = d
        self.X = unit16(rng.standard_normal((N, d)))
        self.Q = unit16(rng.standard_normal((F * REP, d)))
        self.X32, self.Q32 = self.X.astype(np.float32), self.Q.astype(np.float32)  # the exact upcast
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
        """the float32 oracle's PrefilterIndex rows of the batch on the upcast, computed once"""
        key = (sfx, path, k)
        if key not in self._oracle:
            oi = getattr(oracle, "PrefilterIndex" + f32_class(sfx))(self.X32, self.labels)
            self._oracle[key] = oi.batch_search(self.Q32, self.windows(path), len(self.Q), qp(oracle, k))
        return self._oracle[key]
