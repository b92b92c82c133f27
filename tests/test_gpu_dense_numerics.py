"""GPU: the float dense path's proof bound where it decides something -- near ties, extreme scales, common offsets, mixed norms.

For float32 / float16 rows an MFMA score is a three-product split-bf16 approximation of the distance, and a batch's rows are right
only because rerank_query proves d_k + E < cut - E (or rescues, or hands the query back to the scan).  On unit-scale, well-spread
rows the gap between the k-th distance and the cut is hundreds of times E, so any E passes.  The inputs here (numerics_util) make
score order and distance order really disagree, or drive the terms of E to the ends of the fp32 range.  Both dense paths run on
them: shared-window groups and cover groups (`set_dense_windows`).  The contract is the existing one:
  * rows (ids and distance bits) equal the exact scan's on the same index,
  * golden_util.same_rows against the oracle (float16: the float32 oracle on the upcast),
  * an independent float64 check: every returned distance lies within (d + 2) 2^-24 sum|terms| of the float64 distance of the
    returned id (the standard bound of a length-d fp32 sum: three roundings per term, d - 1 additions), and no point of the window
    has a float64 distance below the returned k-th by more than that bound for the point plus that bound for the k-th (for L2,
    where the terms are the distance itself, at most twice the k-th's)."""
import os

import numpy as np
import pytest

import golden_util as gu
import numerics_util as nu

pytestmark = pytest.mark.gpu

ZERO = dict(queries=0, unproven=0, rescued=0, groups=0, tiles=0, passes=0, handover_bytes=0)
PATHS = ("shared", "cover")
U = 2.0 ** -24
FLT_MIN, FLT_MAX = 2.0 ** -126, float(np.finfo(np.float32).max)


def _qp(mod, k=10):
    return mod.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False)


def _elem(sfx):
    return np.float16 if sfx.startswith("Float16") else np.float32


def _note(line):
    print("[dense numerics] " + line)
    out = os.environ.get("DENSE_NUMERICS_COUNTERS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _search(pi, wa, Q, W, k, device):
    """host call, or (device=True) the device-buffer call with fp32 queries and windows as they are"""
    nq = len(Q)
    if not device:
        return pi.batch_search(Q, W, nq, _qp(wa, k))
    import torch
    dev = torch.device("cuda:0")
    tq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    tw = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).to(dev)
    ti = torch.zeros((nq, k), dtype=torch.int32, device=dev)
    td = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    pi.batch_search_device(tq.data_ptr(), tw.data_ptr(), nq, 0, "", _qp(wa, k), ti.data_ptr(), td.data_ptr(), 0)
    return ti.cpu().numpy().view(np.uint32), td.cpu().numpy()


def _run(pi, wa, monkeypatch, path, Q, W, k, device=False, scan_check=None):
    """one batch on the exact scan and on the dense path `path`; scan_check(ids, dists), if given, sees the scan's rows first;
    then the dense rows must be the scan's bit for bit.  Returns the rows and the path's counters."""
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")  # (test hook: no minimum on the batch's scan work for the cover path)
    pi.set_dense_windows(False)
    monkeypatch.setenv("WANN_NO_GEMM", "1")
    ids0, d0 = _search(pi, wa, Q, W, k, device)
    assert pi.counters()["gemm_queries"] == 0 and pi.dense_window_counters() == ZERO
    monkeypatch.delenv("WANN_NO_GEMM")
    if scan_check is not None:
        scan_check(ids0, d0)
    pi.set_dense_windows(path == "cover")
    ids1, d1 = _search(pi, wa, Q, W, k, device)
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
    assert ctr["queries"] == len(Q), (path, ctr)  # every query of these batches is eligible for its path
    return ids1, d1, ctr


class _Float64:
    """float64 distances and error bounds of every (query, point of its family's widest window) pair of a Families batch, of
    the values as the index and the kernel hold them (X in its storage type, Q as passed)"""

    def __init__(self, fam, X, Q, metric):
        self.fam, self.d = fam, X.shape[1]
        self.D, self.B = [], []
        Xf, Qf = X.astype(np.float32), Q.astype(np.float32)
        for f in range(fam.F):
            P, q = Xf[fam.window_rows(f)], Qf[f * nu.REP:(f + 1) * nu.REP]
            self.D.append(nu.dist64(P, q, metric))
            self.B.append((self.d + 2) * U * nu.abs_terms64(P, q, metric))
        self.pos_of = np.empty(fam.n, dtype=np.int64)
        self.pos_of[fam.order] = np.arange(fam.n)

    def check(self, qsel, a, b, ids, dists):
        """qsel: the batch's rows as indices into the Families' queries; [a, b): their windows as positions"""
        fam = self.fam
        for r, qi in enumerate(qsel):
            f, j = fam.family[qi], qi % nu.REP
            pos = self.pos_of[ids[r].astype(np.int64)]
            assert ((pos >= a[r]) & (pos < b[r])).all(), (qi, ids[r], pos, a[r], b[r])
            rel = pos - fam.a[f]
            D, B = self.D[f][j], self.B[f][j]
            err = np.abs(dists[r].astype(np.float64) - D[rel])
            assert (err <= B[rel]).all(), (qi, ids[r], dists[r], D[rel], B[rel])
            lo, hi = a[r] - fam.a[f], b[r] - fam.a[f]
            better = D[lo:hi] < float(dists[r, -1]) - (B[lo:hi] + B[rel[-1]])
            better[rel - lo] = False  # (the returned points themselves)
            assert not better.any(), (qi, np.nonzero(better)[0][:5] + a[r], D[lo:hi][better][:5], dists[r])


def _oracle_rows(oracle, sfx, X, labels, Q, W, k):
    cls = getattr(oracle, "PrefilterIndex" + sfx.replace("Float16", "Float"))
    oi = cls(X.astype(np.float32), labels)
    return oi.batch_search(Q.astype(np.float32), W, len(Q), _qp(oracle, k))


class _Case:
    """one index over X (cast to the class's element type) with the labels of `fam`, and the three row checks of a batch"""

    def __init__(self, oracle, wa, monkeypatch, sfx, fam, X, Q, device=False):
        self.oracle, self.wa, self.mp, self.sfx, self.fam, self.device = oracle, wa, monkeypatch, sfx, fam, device
        self.metric = gu.metric_of(sfx)
        self.X = np.ascontiguousarray(X.astype(_elem(sfx)))
        self.Q = np.ascontiguousarray(Q.astype(np.float32 if device else _elem(sfx)))
        self.pi = getattr(wa, "PrefilterIndex" + sfx)(self.X, fam.labels)
        self.f64 = _Float64(fam, self.X, self.Q, self.metric)

    def run(self, path, k, qsel=None, scan_check=None, rows=True):
        fam = self.fam
        qsel = np.arange(len(self.Q)) if qsel is None else qsel
        a, b = (x[qsel] for x in fam.positions(path))
        W = fam.windows(path)[qsel]
        Q = np.ascontiguousarray(self.Q[qsel])
        ids, dists, ctr = _run(self.pi, self.wa, self.mp, path, Q, W, k, self.device, scan_check)
        if rows:
            eids, edists = _oracle_rows(self.oracle, self.sfx, self.X, fam.labels, Q, W, k)
            ctx = gu.RowContext(self.X.astype(np.float32), fam.labels, Q.astype(np.float32), W, self.metric, "prefilter")
            ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
            assert ok, f"{self.sfx} {path} k={k}: {why}"
            self.f64.check(qsel, a, b, ids, dists)
        return ids, dists, ctr


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sfx,d", nu.NEAR_TIE_CASES)
def test_near_ties(oracle, wa, gpu, monkeypatch, sfx, d, path):
    """Shells of 128 points whose exact distances differ by about 2^-21 relative -- far below the split's 2^-16 --, scattered over
    the window (defeats the selection cut) and contiguous (defeats the per-lane hand-over).  Rows equal; over the shell queries
    unproven + rescued is at least the number of queries for which the score model says the top k cannot lie in the 32 best
    scores; the control queries of the same set keep the cap of a tenth."""
    fam = nu.near_tie_families(d)
    case = _Case(oracle, wa, monkeypatch, sfx, fam, fam.X, fam.Q)
    shell, control = np.nonzero(fam.is_shell)[0], np.nonzero(~fam.is_shell)[0]
    for k in (10, 1, 16):
        ids, dists, ctr = case.run(path, k)
        if (d, case.metric, k) not in _need:  # (the same for both paths)
            _need[d, case.metric, k] = int(fam.outside_keep(case.metric, k)[shell].sum())
        need = _need[d, case.metric, k]
        _, _, cs = case.run(path, k, shell, rows=False)
        _, _, cc = case.run(path, k, control, rows=False)
        _note(f"near ties {sfx} d={d} {path} k={k}: batch {ctr}; shell queries {cs}, model says {need} of {len(shell)} cannot be "
              f"settled; control queries {cc}")
        assert cs["unproven"] + cs["rescued"] >= need, (cs, need)
        if k == 10:
            assert cc["unproven"] <= len(control) // 10, cc


_need = {}
RUNGS = [(0, 0), (-20, -20), (-40, -40), (-50, -50), (-60, 0), (0, -60), (30, 30), (40, 40), (60, 60)]


def _assert_normal(fam, X, Q, metric):
    """every term and every distance the reference forms inside a window is zero or a finite normal fp32 number (in float64)"""
    for f in range(fam.F):
        P = X[fam.window_rows(f)].astype(np.float64)
        for q in Q[f * nu.REP:(f + 1) * nu.REP].astype(np.float64):
            t = np.abs(P * q) if metric == "mips" else (P - q) ** 2
            dist = np.abs(t.sum(axis=1) if metric == "l2" else (P * q).sum(axis=1))
            for v in (t[t > 0], dist[dist > 0], np.abs(t).sum(axis=1)):
                assert v.min() >= FLT_MIN and v.max() <= FLT_MAX, (metric, f, v.min(), v.max())


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("data", ("spread", "shell"))
@pytest.mark.parametrize("sfx", ("FloatEuclidian", "FloatMips"))
def test_scale_ladder(oracle, wa, gpu, monkeypatch, sfx, data, path):
    """Rows scaled by 2^s, queries by 2^t: exact in fp32 while nothing under- or overflows, so the ids are the unscaled run's and
    the distance bits are ldexp(unscaled, s + t) (inner product) / ldexp(unscaled, 2 s) at s = t (L2) -- on the scan's rows first,
    which validates the rung, then on the dense rows.  Rungs with s != t run under L2 with the three row checks alone.  At
    (-40, -40) and (-50, -50) q2 * pmax underflows in fp32, at (40, 40) it overflows: the inner product's E must survive both."""
    fam = nu.ladder_families(data)
    mips = sfx.endswith("Mips")
    base = {}
    for s, t in RUNGS:
        if mips and (s, t) == (60, 60):
            continue  # (the products overflow)
        X, Q = np.ldexp(fam.X, s), np.ldexp(fam.Q, t)
        _assert_normal(fam, X, Q, gu.metric_of(sfx))
        case = _Case(oracle, wa, monkeypatch, sfx, fam, X, Q)
        shift = s + t if mips else 2 * s if s == t else None
        for k in (10, 1, 16) if (s, t) in ((0, 0), (-40, -40)) else (10,):
            def same_as_unscaled(ids, dists, k=k):
                if shift is not None and (s, t) != (0, 0):
                    bids, bd = base[k]
                    assert np.array_equal(np.ldexp(bd, shift).view(np.uint32), dists.view(np.uint32)), (s, t, k)
                    assert np.array_equal(bids, ids), (s, t, k)
            ids, dists, ctr = case.run(path, k, scan_check=same_as_unscaled)
            same_as_unscaled(ids, dists)
            if (s, t) == (0, 0):
                base[k] = (ids, dists)
            _note(f"ladder {sfx} {data} {path} rows 2^{s} queries 2^{t} k={k}: {ctr}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sfx", ("Float16Euclidian", "Float16Mips"))
def test_scale_ladder_float16(oracle, wa, gpu, monkeypatch, sfx, path):
    """float16 rows (the grid values are exact halves): the ladder runs on the queries, through the device-buffer call with fp32
    queries; then rows at the two ends of the half range (largest element 65 504; subnormal halves) with float16 queries."""
    fam = nu.ladder_families("shell")
    mips = sfx.endswith("Mips")
    base = {}
    for t in (0, -20, -40, -60, 30, 40):
        Q = np.ldexp(fam.Q, t)
        _assert_normal(fam, fam.X.astype(np.float16).astype(np.float32), Q, gu.metric_of(sfx))
        case = _Case(oracle, wa, monkeypatch, sfx, fam, fam.X, Q, device=True)
        for k in (10, 1, 16) if t in (0, -40) else (10,):
            def same_as_unscaled(ids, dists, k=k):
                if mips and t != 0:
                    assert np.array_equal(np.ldexp(base[k][1], t).view(np.uint32), dists.view(np.uint32)), (t, k)
                    assert np.array_equal(base[k][0], ids), (t, k)
            ids, dists, ctr = case.run(path, k, scan_check=same_as_unscaled)
            same_as_unscaled(ids, dists)
            if t == 0:
                base[k] = (ids, dists)
            _note(f"ladder {sfx} shell {path} queries 2^{t} (device call) k={k}: {ctr}")
    top = 65504.0 / float(np.abs(fam.X).max())
    for name, X in (("largest element 65504", fam.X * top), ("subnormal halves", np.ldexp(fam.X, -14))):
        X16 = X.astype(np.float16)
        assert np.isfinite(X16).all() and (X16 != 0).all()
        assert np.abs(X16).max() == 65504 if name[0] == "l" else (np.abs(X16.astype(np.float32)) < 2.0 ** -14).mean() > 0.99
        case = _Case(oracle, wa, monkeypatch, sfx, fam, X16, fam.Q)
        ids, dists, ctr = case.run(path, 10)
        _note(f"half range {sfx} {path} {name} k=10: {ctr}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sfx,d", (("FloatEuclidian", 64), ("FloatEuclidian", 200), ("Float16Euclidian", 100)))
def test_common_offset(oracle, wa, gpu, monkeypatch, sfx, d, path):
    """Rows and queries mu 1 + unit-scale noise: |p|^2 - 2 q.p cancels, E grows with mu^2 d while the gaps stay at unit scale.
    Rows equal; the counters per mu are printed (from mu = 64 on E legitimately swamps the gaps: no cap); at mu = 0 the cap."""
    fam = nu.Families(3000 + d, d, ["control"] * 6)
    for mu in (0.0, 4.0, 64.0, 1024.0, 2.0 ** 15):
        case = _Case(oracle, wa, monkeypatch, sfx, fam, (fam.X.astype(np.float64) + mu).astype(np.float32),
                     (fam.Q.astype(np.float64) + mu).astype(np.float32))
        for k in (10, 1, 16) if mu == 4.0 else (10,):
            ids, dists, ctr = case.run(path, k)
            _note(f"offset {sfx} d={d} {path} mu={mu:g} k={k}: {ctr}")
            if mu == 0.0:
                assert ctr["unproven"] <= len(fam.Q) // 10, ctr


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sfx,d", (("FloatEuclidian", 64), ("FloatMips", 100), ("FloatMips", 500), ("Float16Euclidian", 100), ("Float16Mips", 64)))
def test_mixed_norms(oracle, wa, gpu, monkeypatch, sfx, d, path):
    """(a) row norms log-uniform over 2^-20 .. 2^20 (float16: 2^-10 .. 2^10) inside every window; (b) unit-norm rows plus ONE
    row of norm 2^30 (float16: 2^15) outside every window: pmax is the maximum over the whole index, so E is that of the
    outlier -- rows must be equal, what goes back to the scan is printed, not judged; (c) zero rows, zero queries and -0.0
    elements mixed into the batch (the FLT_MIN floor of E)."""
    fam = nu.Families(4000 + d, d, ["control"] * 6)
    rng = np.random.default_rng(d)
    half = sfx.startswith("Float16")
    e = 10 if half else 20
    Xa = (fam.X * 2.0 ** rng.uniform(-e, e, (fam.n, 1))).astype(np.float32)
    case = _Case(oracle, wa, monkeypatch, sfx, fam, Xa, fam.Q)
    for k in (10, 1, 16):
        _note(f"mixed norms {sfx} d={d} {path} (a) log-uniform k={k}: {case.run(path, k)[2]}")
    Xb = fam.X.copy()
    out_pos = nu.SLOT * 3 + 100
    assert not ((fam.a <= out_pos) & (out_pos < fam.b)).any()
    case = _Case(oracle, wa, monkeypatch, sfx, fam, Xb, fam.Q)
    _note(f"mixed norms {sfx} d={d} {path} (b) unit rows k=10: {case.run(path, 10)[2]}")
    Xb[fam.order[out_pos]] *= 2.0 ** (15 if half else 30)
    case = _Case(oracle, wa, monkeypatch, sfx, fam, Xb, fam.Q)
    _note(f"mixed norms {sfx} d={d} {path} (b) one row of norm 2^{15 if half else 30} outside every window k=10: {case.run(path, 10)[2]}")
    Xc, Qc = fam.X.copy(), fam.Q.copy()
    for f in range(fam.F):  # twenty zero rows per window, some written as -0.0; every eighth query zero, every ninth has -0.0 elements
        rows = fam.window_rows(f)[rng.choice(fam.b[f] - fam.a[f] - 2 * nu.REP, 20, replace=False) + nu.REP]
        Xc[rows] = 0.0
        Xc[rows[::2], ::3] = -0.0
    Qc[::8] = 0.0
    Qc[::16, ::2] = -0.0
    Qc[1::9, ::5] = -0.0
    case = _Case(oracle, wa, monkeypatch, sfx, fam, Xc, Qc)
    for k in (10, 16):
        _note(f"mixed norms {sfx} d={d} {path} (c) zero rows and queries k={k}: {case.run(path, k)[2]}")
