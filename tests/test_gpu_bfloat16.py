"""GPU: bfloat16 point sets (include/wann.h WANN_DTYPE_BF16 = 5) against the oracle and the float32 path on the points rounded
to bfloat16.  A bfloat16 widens to float32 by a shift, exactly, and the kernels score it in the float32 path's arithmetic, so
ids, distance bits and the reference's operation counters must equal those of float32 on the upcast rows, in every
beam-search core -- over float32's whole exponent range, which binary16 cannot hold."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
from util import REPO, distinct_labels, sift_like, unit_mixture, windows

pytestmark = pytest.mark.gpu
BF16 = 5


def _qp(mod, beam, mult=1, k=10, max_beam=10000, verbose=False):
    return mod.QueryParams(k, beam, 1.35, 10_000_000, 10_000, mult, max_beam, None, verbose)


def _rounded(wa, gen, n, d, seed, scale=1.0):
    """a generator's data and 96 queries, scaled (by a power of two) and rounded to bfloat16: float32 arrays"""
    g = gen(n, d, seed)
    return wa.bfloat16_round(g(n) * np.float32(scale)), wa.bfloat16_round(g(96) * np.float32(scale))


def _raw_case(oracle, wa, metric, X32, Q32, R, beams, start, sn, qids):
    """X32: bfloat16-exact float32 rows; the kernel gets their bit patterns, the oracle the float32 values"""
    d = X32.shape[1]
    bits = wa.bfloat16_bits(X32)
    assert np.array_equal(bits.astype(np.uint32) << 16, X32.view(np.uint32))
    Xp = oracle.pad_rows(X32)
    rows = oracle.vamana_build(Xp, d, metric, start, sn, R, 2 * R, 1.0)
    bad = []
    for beam in beams:
        ids, dists, sizes, hops, cmps = wa.raw_beam_search_typed(metric, BF16, bits, rows, start, Q32, qids, beam)
        for i in range(len(Q32)):
            oi, od, vi, vd, dc = oracle.beam_search(rows, Xp, d, metric, start, Q32[i], int(qids[i]), beam)
            m = int(sizes[i])
            if not (m == len(oi) and np.array_equal(ids[i, :m], oi) and np.array_equal(dists[i, :m].view(np.uint32), od.view(np.uint32))
                    and int(hops[i]) == len(vi) and int(cmps[i]) == dc):
                bad.append((beam, i, m, len(oi), int(hops[i]), len(vi), int(cmps[i]), dc))
    assert not bad, (len(bad), bad[:5])


# ------------------------------------------------------------------------------------------
# raw kernel: every beam-search core on bfloat16 rows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,gen,d", [(0, sift_like, 128), (1, unit_mixture, 100), (0, unit_mixture, 40),
                                          (1, unit_mixture, 512), (0, unit_mixture, 200)])
def test_raw_beam_search_bfloat16_matches_oracle(oracle, wa, gpu, metric, gen, d):
    n = 3000
    X, Q = _rounded(wa, gen, n, d, 11)
    qids = np.arange(len(Q), dtype=np.int64)
    qids[::3] += 700  # some queries carry an id that names a node of the partition (self-skip quirk)
    _raw_case(oracle, wa, metric, X, Q, 32, (1, 10, 64, 65, 160, 700, 2500), 500, 2000, qids)


@pytest.mark.parametrize("env", [{"WANN_FORCE_GENERAL": "1"}, {"WANN_OLD_GENERAL": "1"}, {"WANN_RAW_BIG_LDS": "1"},
                                 {"WANN_RAW_BIG_LDS": "1", "WANN_FORCE_GENERAL": "1"},
                                 {"WANN_RAW_BIG_LDS": "1", "WANN_FORCE_GENERAL": "1", "WANN_NO_HELPER": "1"}],
                         ids=lambda e: "+".join(sorted(e)))
@pytest.mark.parametrize("metric,gen,d", [(0, sift_like, 128), (1, unit_mixture, 100)])
def test_raw_beam_search_bfloat16_core_variants(oracle, wa, gpu, monkeypatch, env, metric, gen, d):
    X, Q = _rounded(wa, gen, 5000, d, 12)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    qids = np.arange(len(Q), dtype=np.int64) + 10**6
    _raw_case(oracle, wa, metric, X, Q, 32, (16, 100, 300, 1000), 300, 4500, qids)


def test_raw_beam_search_bfloat16_wide_rows(oracle, wa, gpu):
    X, Q = _rounded(wa, sift_like, 3000, 64, 13)
    qids = np.arange(len(Q), dtype=np.int64) + 10**6
    _raw_case(oracle, wa, 0, X, Q, 96, (10, 100, 400), 200, 2500, qids)


@pytest.mark.parametrize("metric", [0, 1])
def test_raw_beam_search_bfloat16_tie_heavy(oracle, wa, gpu, metric):
    """values k / 4, k < 13 (bfloat16-exact) and duplicate rows: equal distances everywhere"""
    n, d = 4000, 6
    rng = np.random.default_rng(99)
    X = (rng.integers(0, 13, size=(n, d)) / 4.0).astype(np.float32)
    X[rng.choice(n, 600, replace=False)] = X[rng.choice(n, 600)]
    Q = (rng.integers(0, 13, size=(48, d)) / 4.0).astype(np.float32)
    Q[::4] = X[rng.choice(n, 12)]
    assert np.array_equal(wa.bfloat16_round(X), X)
    qids = np.arange(len(Q), dtype=np.int64) + 10**6
    _raw_case(oracle, wa, metric, X, Q, 32, (20, 64, 130, 250, 640, 2000), 200, 3600, qids)


@pytest.mark.parametrize("metric,gen,d,scale", [(0, sift_like, 64, 2.0 ** 18), (1, unit_mixture, 100, 2.0 ** 18),
                                                (0, unit_mixture, 40, 2.0 ** -60), (1, unit_mixture, 96, 2.0 ** -60)],
                         ids=["l2-2p18", "mips-2p18", "l2-2m60", "mips-2m60"])
def test_raw_beam_search_bfloat16_range(oracle, wa, gpu, metric, gen, d, scale):
    """rows binary16 cannot hold: scaled by 2^18 (beyond 65504) and by 2^-60 (below 2^-24); the squares stay normal float32"""
    X, Q = _rounded(wa, gen, 3000, d, 14, scale)
    amax = float(np.abs(X).max())
    assert (amax > 65504.0) if scale > 1 else (amax < 2.0 ** -24)
    norm2 = (X.astype(np.float64) ** 2).sum(axis=1)  # (squared norms, and with them the distances between rows, are normal float32)
    assert np.isfinite(np.float32(norm2.max() * 4)) and norm2.min() > 2.0 ** -126
    qids = np.arange(len(Q), dtype=np.int64) + 10**6
    _raw_case(oracle, wa, metric, X, Q, 32, (10, 100, 700), 300, 2500, qids)


# ------------------------------------------------------------------------------------------
# index level: every kind x both metrics against the oracle on the upcast points
# ------------------------------------------------------------------------------------------
CASES = [
    ("VamanaRangeFilterTreeIndex", "Euclidian", sift_like, 128, 6000, dict(cutoff=500, split_factor=2)),
    ("VamanaRangeFilterTreeIndex", "Mips", unit_mixture, 96, 6000, dict(cutoff=300, split_factor=4)),
    ("SuperOptimizedPostfilterTreeIndex", "Mips", unit_mixture, 100, 5000, dict(cutoff=400, split_factor=2, shift_factor=0.5)),
    ("SuperOptimizedPostfilterTreeIndex", "Euclidian", sift_like, 96, 5000, dict(cutoff=300, split_factor=2.5, shift_factor=0.3)),
    ("PostfilterVamanaIndex", "Euclidian", unit_mixture, 64, 4000, dict()),
    ("PostfilterVamanaIndex", "Mips", unit_mixture, 100, 4000, dict()),
    ("RangeFilterTreeIndex", "Euclidian", sift_like, 48, 4000, dict(cutoff=300, split_factor=2)),
    ("RangeFilterTreeIndex", "Mips", unit_mixture, 40, 4000, dict(cutoff=300, split_factor=2)),
    ("PrefilterIndex", "Mips", unit_mixture, 100, 4000, dict()),
    ("PrefilterIndex", "Euclidian", sift_like, 128, 4000, dict()),
]


@pytest.mark.parametrize("kind,metric,gen,d,n,kw", CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_bfloat16_index_matches_oracle(oracle, wa, gpu, tmp_path, kind, metric, gen, d, n, kw):
    nq = 300
    g = gen(n, d, 21)
    X32, Q32 = wa.bfloat16_round(g(n)), wa.bfloat16_round(g(nq))
    labels = distinct_labels(n, 3)
    cache = str(tmp_path) + "/"
    labkw = "filters" if kind == "PostfilterVamanaIndex" else "filter_values"
    pi = getattr(wa, kind + "BFloat16" + metric)(X32, **{labkw: labels}, build_params=wa.BuildParams(32, 64, 1.0, cache), **kw)
    oi = getattr(oracle, kind + "Float" + metric)(X32, **{labkw: labels}, build_params=oracle.BuildParams(32, 64, 1.0, cache), **kw)
    assert pi.half_rows() is False and pi.set_half_rows(True) is False
    tree = kind.endswith("RangeFilterTreeIndex")
    methods = ("optimized_postfilter", "fenwick", "three_split") if tree else ("",)
    fractions = [-9, -7, -6, -4, -2, 0] if kind != "PrefilterIndex" else [-6, -3, -1]
    ctx = lambda W: gu.RowContext(X32, labels, Q32, W, gu.metric_of(metric))  # noqa: E731
    for method in methods:
        for p in fractions:
            W = windows(labels, nq, p, seed=50 + p)
            for beam, mult in [(10, 1), (40, 2), (200, 1)]:
                a = (W, nq) + ((method,) if tree else ())
                ids, dists = pi.batch_search(Q32, *a, _qp(wa, beam, mult))
                eids, edists = oi.batch_search(Q32, *a, _qp(oracle, beam, mult))
                tie = kind in gu.TIE_AWARE_KINDS or method != "optimized_postfilter" or p <= -6
                ok, why = gu.same_rows(eids, edists, ids, dists, tie, ctx(W))
                assert ok, f"{kind}BFloat16{metric} {method} p={p} beam={beam} mult={mult}: {why}"
                c, oc = pi.counters(), oi.last_counters
                assert c["beam_searches"] == oc["searches"] and c["hops"] == oc["hops"], (method, p, beam)
                assert c["dist_cmps"] + c["brute_rows"] == oc["dist_cmps"], (method, p, beam)
                assert c["gemm_queries"] == 0


@pytest.mark.parametrize("kind,metric,gen,d,kw", [
    ("VamanaRangeFilterTreeIndex", "Euclidian", sift_like, 128, dict(cutoff=500, split_factor=2)),
    ("SuperOptimizedPostfilterTreeIndex", "Mips", unit_mixture, 100, dict(cutoff=400, split_factor=2, shift_factor=0.5))])
def test_bfloat16_equals_float32_index_on_every_call(wa, gpu, tmp_path, kind, metric, gen, d, kw):
    """the bfloat16 index against the float32 index on the upcast points: the host call, the device call with fp32 queries, the
    asynchronous call and the per-query-id call give the float32 index's rows, bit for bit; the GPU builder's graph files equal
    the float32 build's; only the vector store shrinks"""
    torch = pytest.importorskip("torch")
    n, nq = 30000, 600
    g = gen(n, d, 31)
    X32, Q32 = wa.bfloat16_round(g(n)), wa.bfloat16_round(g(nq))
    labels = distinct_labels(n, 9)
    hdir, fdir = str(tmp_path / "h") + "/", str(tmp_path / "f") + "/"
    os.makedirs(hdir), os.makedirs(fdir)
    h = getattr(wa, kind + "BFloat16" + metric)(X32, labels, build_params=wa.BuildParams(32, 64, 1.0, hdir), **kw)
    f = getattr(wa, kind + "Float" + metric)(X32, labels, build_params=wa.BuildParams(32, 64, 1.0, fdir), **kw)
    names = sorted(os.listdir(hdir))
    assert names and names == sorted(os.listdir(fdir))
    for name in names:
        assert open(hdir + name, "rb").read() == open(fdir + name, "rb").read(), name
    row32, row16 = -(-d * 4 // 64) * 64, -(-d * 2 // 64) * 64
    assert f.device_bytes() - h.device_bytes() == n * (row32 - row16)
    assert h.half_rows() is False
    tree = kind.endswith("RangeFilterTreeIndex")
    dev = torch.device("cuda:0")
    tq = torch.from_numpy(Q32).to(dev)
    # a torch.bfloat16 tensor passes through .float().numpy() exactly
    assert np.array_equal(torch.from_numpy(Q32).to(torch.bfloat16).float().numpy().view(np.uint32), Q32.view(np.uint32))
    for p in (-9, -7, -5, -3, 0):
        W = windows(labels, nq, p, 70 + p).astype(np.float32)
        for beam, mult in ((10, 1), (40, 2)):
            qp = _qp(wa, beam, mult)
            a = ("optimized_postfilter",) if tree else ()
            fi, fd = f.batch_search(Q32, W, nq, *a, qp)
            fc = f.counters()
            hi, hd = h.batch_search(Q32, W, nq, *a, qp)
            hc = h.counters()
            assert np.array_equal(hi, fi) and np.array_equal(hd.view(np.uint32), fd.view(np.uint32)), (p, beam)
            for key in ("beam_searches", "hops", "dist_cmps", "brute_rows"):
                assert hc[key] == fc[key], (p, beam, key)
            method = a[0] if tree else ""
            tw = torch.from_numpy(W).to(dev)
            ti = torch.empty((nq, 10), dtype=torch.int32, device=dev)
            td = torch.empty((nq, 10), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            h.batch_search_device(tq.data_ptr(), tw.data_ptr(), nq, 0, method, qp, ti.data_ptr(), td.data_ptr(), 0)
            assert np.array_equal(ti.cpu().numpy().view(np.uint32), fi) and np.array_equal(td.cpu().numpy(), fd), ("device", p)
            ti.zero_()
            td.zero_()
            t = h.batch_search_device_async(tq.data_ptr(), tw.data_ptr(), nq, 0, method, qp, ti.data_ptr(), td.data_ptr(), 0)
            h.wait(t)
            assert np.array_equal(ti.cpu().numpy().view(np.uint32), fi) and np.array_equal(td.cpu().numpy(), fd), ("async", p)
            qids = torch.arange(nq, dtype=torch.int64, device=dev)
            ti.zero_()
            td.zero_()
            torch.cuda.synchronize()
            h.batch_search_device_ids(tq.data_ptr(), tw.data_ptr(), nq, qids.data_ptr(), method, qp, ti.data_ptr(), td.data_ptr(), 0)
            assert np.array_equal(ti.cpu().numpy().view(np.uint32), fi) and np.array_equal(td.cpu().numpy(), fd), ("ids", p)


def test_bfloat16_subnormal_elements_on_the_device(wa, gpu):
    """bfloat16-subnormal elements (multiples of 2^-133) widen by integer instructions: no denormal mode can flush them.  Queries
    2^100 e_i make every returned inner product a NORMAL float32 that exposes one element exactly: k * 2^-33."""
    n, d, nq = 2000, 16, 32
    rng = np.random.default_rng(4)
    k = rng.integers(-127, 128, size=(n, d))
    X = (k * 2.0 ** -133).astype(np.float32)
    assert np.array_equal(wa.bfloat16_round(X), X) and (np.abs(X) < 2.0 ** -126).all() and (X != 0).any()
    Q = np.zeros((nq, d), dtype=np.float32)
    Q[np.arange(nq), np.arange(nq) % d] = np.float32(2.0 ** 100) * np.where(np.arange(nq) < d, 1, -1).astype(np.float32)
    labels = distinct_labels(n, 5)
    b = wa.PrefilterIndexBFloat16Mips(X, labels)
    f = wa.PrefilterIndexFloatMips(X, labels)
    for p in (-3, 0):
        W = windows(labels, nq, p, 9)
        bi, bd = b.batch_search(Q, W, nq, _qp(wa, 10))
        fi, fd = f.batch_search(Q, W, nq, _qp(wa, 10))
        assert np.array_equal(bd.view(np.uint32), fd.view(np.uint32)), p
        ok, why = gu.same_rows(fi, fd, bi, bd, True, gu.RowContext(X, labels, Q, W, gu.metric_of("Mips")))
        assert ok, why
        # every returned distance is minus the element its query exposes, exactly: -(+-k) 2^-33, a normal float32
        col, sgn = np.arange(nq) % d, np.where(np.arange(nq) < d, 1, -1)
        want = (-(sgn[:, None] * k[bi.astype(np.int64), col[:, None]]) * 2.0 ** -33).astype(np.float32)
        assert np.array_equal(bd, want) and (bd != 0).any(), p


_VERBOSE_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%(repo)r, %(repo)r + "/tests"]
import rangefilteredann_amd, window_ann as wa
from util import distinct_labels, unit_mixture, windows
n, d, nq = 4000, 100, 24
g = unit_mixture(n, d, 8)
X, Q = wa.bfloat16_round(g(n)), wa.bfloat16_round(g(nq))
labels = distinct_labels(n, 2)
W = windows(labels, nq, -6, 4)
for cls in ("Float", "BFloat16"):
    idx = getattr(wa, "VamanaRangeFilterTreeIndex" + cls + "Mips")(X, labels, cutoff=400, split_factor=2,
                                                                  build_params=wa.BuildParams(32, 64, 1.0, ""))
    sys.stdout.flush()
    print("=====BEGIN", flush=True)
    idx.batch_search(Q, W, nq, "optimized_postfilter", wa.QueryParams(10, 10, 1.35, 10**7, 10**4, 2, 10000, None, True))
    sys.stdout.flush()
    print("=====END", flush=True)
"""


def test_bfloat16_verbose_dump_equals_float32(gpu):
    """QueryParams.verbose on a bfloat16 index prints, line for line, what the float32 index on the upcast points prints"""
    p = subprocess.run([sys.executable, "-c", _VERBOSE_CHILD % {"repo": REPO}], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    parts = [b.split("=====END", 1)[0] for b in p.stdout.split("=====BEGIN")[1:]]
    assert len(parts) == 2 and parts[0].strip(), p.stdout[-2000:]
    assert parts[0] == parts[1]
