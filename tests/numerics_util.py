"""Inputs on which the float dense path's score order and the exact distance order disagree, and a numpy model of the score
kernels' arithmetic that is good enough to RANK points with (tests/test_near_tie_inputs.py, tests/test_gpu_dense_numerics.py).

The model is for choosing inputs: it says for which queries the split-bf16 scores cannot settle the top k.  No GPU test
compares kernel output with it; the references there are the exact scan, the oracle and float64."""
import numpy as np

KEEP = 32        # kSelect: the candidates k_rerank keeps per query
BLOCK = 2048     # kGemmPointChunk
SLOT = 2 * BLOCK  # positions of the label order that one family of queries owns
REP = 40         # queries per family: >= 16 for a shared-window group, >= 32 per block for a cover group
SHELL = 128


def bf16(x):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split(x):
    """x = hi + lo + (what the score kernels drop): hi = bf16(x), lo = bf16(x - hi)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16(x)
    return hi, bf16(x - hi)


def emulated_scores(P, Q, metric):
    """scores of the points P (m, d) for the queries Q (nq, d), (nq, m): qh ph + qh pl + ql ph accumulated in float64;
    -s under the inner product, fl32(|p|^2) - 2 s under L2 (|q|^2 is left out, as in the kernel)"""
    ph, pl = (a.astype(np.float64) for a in split(P))
    qh, ql = (a.astype(np.float64) for a in split(Q))
    s = qh @ ph.T + qh @ pl.T + ql @ ph.T
    if metric == "mips":
        return -s
    p2 = (P.astype(np.float64) ** 2).sum(axis=1).astype(np.float32).astype(np.float64)
    return p2[None, :] - 2.0 * s


def dist64(P, Q, metric):
    """float64 distances of the float32 (or float16) values as they are, (nq, m)"""
    p, q = P.astype(np.float64), Q.astype(np.float64)
    if metric == "mips":
        return -(q @ p.T)
    return np.stack([((p - qi) ** 2).sum(axis=1) for qi in q])


def abs_terms64(P, Q, metric):
    """sum of the absolute values of the d terms of each distance, (nq, m): what the rounding error of an fp32 sum scales with
    (under L2 the terms are squares: the distance itself)"""
    if metric == "mips":
        return np.abs(Q.astype(np.float64)) @ np.abs(P.astype(np.float64)).T
    return dist64(P, Q, metric)


def outside_keep(P, Q, metric, k, keep=KEEP):
    """per query: True where the float64 top k of P is NOT contained in the `keep` best emulated scores -- the selection cannot
    hold the true top k there, whatever the placement of the points in the window is"""
    sc = emulated_scores(P, Q, metric)
    dd = dist64(P, Q, metric)
    out = np.zeros(len(Q), dtype=bool)
    for i in range(len(Q)):
        top = np.argsort(dd[i], kind="stable")[:k]
        best = np.argsort(sc[i], kind="stable")[:keep]
        out[i] = not set(top.tolist()) <= set(best.tolist())
    return out


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def on_grid(x, h, lo):
    """multiples of h with magnitudes of at least lo: differences of two such values are 0 or at least h, so that a ladder of
    power-of-two scales keeps every product and every squared difference a normal fp32 number down to small scales"""
    m = np.maximum(np.rint(np.abs(x) / h) * h, lo)
    return np.where(x < 0, -m, m)


class Families:
    """A point set and a batch made of families of REP queries.  Family f owns positions [SLOT f, SLOT (f + 1)) of the label order
    and a window [a_f, b_f) inside them; kind[f] is "scattered", "contiguous" or "control".  A shell family has a centre c_f of
    unit norm at its SHELL shell positions, rows c_f + sigma |c_f| g (g standard normal), and queries c_f + 0.5 u (u a unit
    vector): the shell is by far the best of the window for each of them under both metrics, and its members' exact distances
    differ by about sigma.  "scattered": shell positions drawn from the whole window (at most one or two per 64-position block);
    "contiguous": 128 consecutive positions, for even f one 128-position step, for odd f the halves of two.  Control families
    have random unit queries.  Everything else is unit-norm Gaussian rows.  grid=True puts everything but the shells' sigma g on
    a grid (on_grid) for the scale ladder.

    windows("shared"): every query of a family has the window [a_f, b_f); windows("cover"): query j has [a_f + j, b_f - j), no two
    alike (the shell lies inside all of them)."""

    def __init__(self, seed, d, kinds, sigma=2.0 ** -21, grid=False, shell=SHELL):
        rng = np.random.default_rng(seed)
        self.d, self.kind, self.F = d, list(kinds), len(kinds)
        F = self.F
        self.n = n = F * SLOT + 64  # (the tail: no window reaches the last point, which the reference's scan never returns)
        h, lo = 2.0 ** -12, 2.0 ** -6
        X = _unit(rng.standard_normal((n, d)))
        if grid:
            X = on_grid(X, h, lo)
        self.order = order = rng.permutation(n)  # order[p] = the row at position p of the label order
        self.labels = np.empty(n, dtype=np.float32)
        self.labels[order] = np.arange(n, dtype=np.float32)
        self.a = SLOT * np.arange(F) + 512 + rng.integers(0, 128, F)
        self.a[::3] -= self.a[::3] % 128
        self.b = self.a + rng.integers(1700, 3000, F)  # (every window of a family reaches into its second block)
        Q = _unit(rng.standard_normal((F * REP, d)))
        if grid:
            Q = on_grid(Q, h, lo)
        self.shell_pos = {}
        for f, kd in enumerate(self.kind):
            if kd == "control":
                continue
            c = _unit(rng.standard_normal(d))
            u = 0.5 * _unit(rng.standard_normal((REP, d)))
            if grid:
                c, u = on_grid(c, h, lo), on_grid(u, h, 2.0 ** -8)
            c32 = c.astype(np.float32).astype(np.float64)
            inner = np.arange(self.a[f] + REP, self.b[f] - REP)
            if kd == "scattered":
                pos = np.sort(rng.choice(inner, shell, replace=False))
            else:
                s0 = inner[0] + 128 - inner[0] % 128 + (64 if f % 2 else 0)
                pos = np.arange(s0, s0 + shell)
            X[order[pos]] = c32 + sigma * np.linalg.norm(c32) * rng.standard_normal((shell, d))
            Q[f * REP:(f + 1) * REP] = on_grid(c32 + u, h, h) if grid else c32 + u  # (on the grid: no element is zero)
            self.shell_pos[f] = pos
        self.X, self.Q = X.astype(np.float32), Q.astype(np.float32)
        self.family = np.repeat(np.arange(F), REP)
        self.is_shell = np.array([self.kind[f] != "control" for f in self.family])

    def positions(self, path):
        j = np.tile(np.arange(REP), self.F) if path == "cover" else 0
        return self.a[self.family] + j, self.b[self.family] - j

    def windows(self, path):
        a, b = self.positions(path)
        return np.stack([a - 0.5, b - 0.5], 1).astype(np.float64)

    def window_rows(self, f):
        """rows of the family's widest window, in label order"""
        return self.order[self.a[f]:self.b[f]]

    def outside_keep(self, metric, k, X=None, Q=None):
        """outside_keep() per query (False for control queries' families is NOT assumed: they are computed too).  The family's
        widest window is used for all of its queries: the cover path's narrower windows drop background rows only."""
        X = self.X if X is None else X
        Q = self.Q if Q is None else Q
        out = np.zeros(len(Q), dtype=bool)
        for f in range(self.F):
            sl = slice(f * REP, (f + 1) * REP)
            out[sl] = outside_keep(X[self.window_rows(f)], Q[sl], metric, k)
        return out


# what the GPU tests run on; tests/test_near_tie_inputs.py checks on the CPU that these very inputs bite
NEAR_TIE_CASES = [("FloatEuclidian", 64), ("FloatMips", 100), ("FloatMips", 200), ("FloatEuclidian", 500)]  # narrow, narrow, _wide<2>, _wide4
LADDER_D = 64


def near_tie_families(d):
    return Families(1000 + d, d, ["scattered", "contiguous", "control"] * 4)


def ladder_families(data, d=LADDER_D):
    """the scale ladder's two sets, on the grid: "shell" (two scattered, two contiguous and two control families) and "spread"
    (six control families: well-spread rows only)"""
    kinds = ["scattered", "contiguous", "control"] * 2 if data == "shell" else ["control"] * 6
    return Families(2000 + d, d, kinds, grid=True)
