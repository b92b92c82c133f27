"""GPU: the window maxima of the dense proof (`set_dense_window_norms`) at the edges of their table, and the trimmed centre.

If `window_norm_max` returns too little, the proof certifies queries it has no right to certify, the rows still come out right on
well-spread data and the only symptom is a counter that is too good.  So these tests hold the COUNTERS to what the code must do
with a row of a huge norm (2^30; float16: 2^15; float8: 64 times the others) at chosen positions of window_edge_util's sites:

  * inside a window -- at its first and last position, where the lookup's first run ends, in the first block that only the second
    run covers and the last that only the first run covers -- no query of the window may be proven: with pmax = 2^60 the bound
    exceeds every gap and the rescue is not entered, so unproven == REP exactly;
  * one position outside the covering blocks, on both sides: every counter of every site equals that of the same data without the
    rows -- the lookup reads no block too many, and the table is the same from run to run.

The sites reach table levels 4 .. 8, block-aligned and unaligned ends and the partial last block.  Every batch's rows are the
same index's exact scan bit for bit (test_gpu_dense_numerics._run); the full batches pass golden_util.same_rows against the
oracle too.  Further down: the other float types, the inner product, k = 17, the centred table, the trimmed centre on either
side of n / 4 outlying rows, the switches flipped on one index in another order than its buffers were built, the tree's route."""
import os

import numpy as np
import pytest

import golden_util as gu
import numerics_util as nu
import window_edge_util as we
from test_gpu_dense_numerics import PATHS, _elem, _oracle_rows, _qp, _run
from test_gpu_dense_window_norms import _UpcastOracle
from util import pos_windows, random_rows

pytestmark = pytest.mark.gpu
REP = we.REP
SITE33, SITE65 = 1, 5
assert we.SITES[SITE33][0] == 33 and we.SITES[SITE65][0] == 65


def _note(line):
    print("[dense window edges] " + line)
    out = os.environ.get("DENSE_WINDOW_EDGES_COUNTERS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


class _Index:
    """one PrefilterIndex over the sites' rows with the placement's rows (and the tail's) scaled up, and its batches"""

    def __init__(self, oracle, wa, sfx, d, placement, mu=0.0, tail_share=None, window_norms=True, centred=False):
        key = (d, tail_share)
        if key not in _sites:
            _sites[key] = we.Sites(5000 + d, d, tail_share)
        self.sites = st = _sites[key]
        self.oracle, self.wa, self.sfx, self.placement, self.metric = _UpcastOracle(oracle), wa, sfx, placement, gu.metric_of(sfx)
        X, Q = ((a.astype(np.float64) + mu).astype(np.float32) for a in (st.X, st.Q))
        big = 2.0 ** (15 if sfx.startswith("Float16") else 30)
        if sfx.startswith("BFloat16"):
            X, Q = nu.bf16(X), nu.bf16(Q)
        if sfx.startswith("Float8"):  # (elements of about 8 / sqrt(d): E4M3's normal range; the outliers stay within 448)
            X, Q, big = wa.float8_round(X * np.float32(8)), wa.float8_round(Q * np.float32(8)), 64.0
        rows = st.order[np.concatenate([st.all_outliers(placement), st.tail_pos])]
        X[rows] *= np.float32(big)
        assert np.abs(X[rows]).max(initial=0) <= (448 if sfx.startswith("Float8") else 65504 if sfx.startswith("Float16") else np.inf)
        self.X, self.Q = np.ascontiguousarray(X.astype(_elem(sfx))), np.ascontiguousarray(Q.astype(_elem(sfx)))
        self.pi = getattr(wa, "PrefilterIndex" + sfx)(self.X, st.labels)
        self.switch(window_norms, centred)
        self.seen = {}

    def switch(self, window_norms, centred):
        assert self.pi.set_dense_window_norms(window_norms) is window_norms and self.pi.set_dense_centred(centred) is centred
        self.state = (window_norms, centred)

    def run(self, mp, path, sites, k=10, rows=False):
        """the batch of these sites' queries: rows bit-equal to the scan's (and, rows=True, right by the oracle); the counters"""
        st = self.sites
        q = st.queries(sites)
        a, b = (x[q] for x in st.positions(path, self.placement))
        Q, W = np.ascontiguousarray(self.Q[q]), pos_windows(a, b)
        ids, dists, ctr = _run(self.pi, self.wa, mp, path, Q, W, k)
        if rows:
            eids, edists = _oracle_rows(self.oracle, self.sfx, self.X, st.labels, Q, W, k)
            ctx = gu.RowContext(self.X.astype(np.float32), st.labels, Q.astype(np.float32), W, self.metric, "prefilter")
            ok, why = gu.same_rows(eids, edists, ids, dists, True, ctx)
            assert ok, f"{self.sfx} {self.placement} {path} k={k}: {why}"
        return ctr

    def per_site(self, mp, path, sites, k=10):
        """{site: (unproven, rescued)} of one sub-batch per site, in the index's present state (kept: a state's counters are taken once)"""
        out = {}
        for s in sites:
            memo = (self.state, path, s, k)
            if memo not in self.seen:
                ctr = self.run(mp, path, [s], k)
                self.seen[memo] = (ctr["unproven"], ctr["rescued"])
            out[s] = self.seen[memo]
        return out


_sites = {}


@pytest.fixture(scope="module")
def index(oracle, wa, gpu):
    """index(sfx, d, placement, ...): built once per module"""
    made = {}

    def get(sfx, d, placement, **kw):
        key = (sfx, d, placement, tuple(sorted(dict(dict(mu=0.0, tail_share=None, window_norms=True, centred=False), **kw).items())))
        if key not in made:
            made[key] = _Index(oracle, wa, sfx, d, placement, **kw)
        return made[key]

    yield get
    made.clear()


def _show(st, ctrs):
    return ", ".join(f"{int(st.m[s])} blocks: unproven {u} rescued {r}" for s, (u, r) in ctrs.items())


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("placement", we.PLACEMENTS)
def test_rows(index, monkeypatch, placement, path):
    """the full batch of every placement's index: the scan's rows, and the oracle's"""
    ix = index("FloatEuclidian", 64, placement)
    ctr = ix.run(monkeypatch, path, ix.sites.sites_of(path), rows=True)
    _note(f"{placement} {path} full batch: {ctr}")


@pytest.mark.parametrize("path", PATHS)
def test_clean_sites_are_proven(index, monkeypatch, path):
    """the precondition of everything below: without an outlier at least half of every site's queries are proven"""
    ix = index("FloatEuclidian", 64, "clean")
    ctrs = ix.per_site(monkeypatch, path, ix.sites.sites_of(path))
    _note(f"clean {path}: {_show(ix.sites, ctrs)}")
    assert all(u <= REP // 2 for u, _ in ctrs.values()), ctrs


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("placement", we.IN_WINDOW)
def test_outlier_inside_every_window(index, monkeypatch, placement, path):
    ix = index("FloatEuclidian", 64, placement)
    sites = ix.sites.sites_of(path, placement)
    assert len(sites) >= 6
    ctrs = ix.per_site(monkeypatch, path, sites)
    _note(f"{placement} {path}: {_show(ix.sites, ctrs)}")
    assert all(u == REP for u, _ in ctrs.values()), ctrs


@pytest.mark.parametrize("path", PATHS)
def test_outlier_one_position_outside_the_cover(index, monkeypatch, path):
    clean, out = index("FloatEuclidian", 64, "clean"), index("FloatEuclidian", 64, "outside")
    sites = out.sites.sites_of(path)
    want, got = clean.per_site(monkeypatch, path, sites), out.per_site(monkeypatch, path, sites)
    _note(f"outside {path}: {_show(out.sites, got)}")
    assert got == want, (got, want)


# (k = 17 is rerank_query_large, asked of a shared-window batch)
OTHER = [("FloatMips", 100, {}, PATHS), ("Float16Euclidian", 64, {}, PATHS), ("BFloat16Euclidian", 64, {}, PATHS), ("Float8Euclidian", 64, {}, PATHS),
         ("FloatEuclidian", 64, dict(k=17), ("shared",)), ("FloatEuclidian", 64, dict(mu=4.0, centred=True), PATHS)]
OTHER = [pytest.param(sfx, d, how, path, id="-".join([sfx, str(d)] + [f"{a}={b:g}" for a, b in how.items()] + [path]))
         for sfx, d, how, paths in OTHER for path in paths]


@pytest.mark.parametrize("placement", ("last", "second_only"))
@pytest.mark.parametrize("sfx,d,how,path", OTHER)
def test_other_routes_and_types(index, monkeypatch, sfx, d, how, path, placement):
    """the inner product, the float16 / bfloat16 / float8 units, rerank_query_large (k = 17) and the table over the centred
    norms, on the sites of 33 and 65 blocks"""
    how = dict(how)
    k = how.pop("k", 10)
    ix = index(sfx, d, placement, **how)
    if k > 16:
        assert ((ix.sites.hi - ix.sites.lo)[[SITE33, SITE65]] >= 96 * k).all() and ix.pi.set_dense_large_k(True) is True
    ix.run(monkeypatch, path, [SITE33, SITE65], k, rows=True)
    ctrs = ix.per_site(monkeypatch, path, [SITE33, SITE65], k)
    _note(f"{sfx} d={d} {how} k={k} {placement} {path}: {_show(ix.sites, ctrs)}")
    assert all(u == REP for u, _ in ctrs.values()), ctrs


@pytest.mark.parametrize("path", PATHS)
def test_centred_outlier_one_position_outside(index, monkeypatch, path):
    """both switches at mu = 4: about twenty of the rows are trimmed from the centre, the table is the one over the centred norms"""
    ix = index("FloatEuclidian", 64, "outside", mu=4.0, centred=True)
    ix.run(monkeypatch, path, [SITE33, SITE65], rows=True)
    ctrs = ix.per_site(monkeypatch, path, [SITE33, SITE65])
    _note(f"centred mu=4 outside {path}: {_show(ix.sites, ctrs)}")
    assert all(u <= REP // 10 for u, _ in ctrs.values()), ctrs


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("share", ((1, 5), (3, 10)))
def test_trimmed_centre_either_side_of_a_quarter(index, monkeypatch, share, path):
    """t rows of one huge norm M at the end of the label order, both switches, mu = 4.  The centre leaves out the rows above
    kTrimFactor = 4 times the mean squared norm, about 4 (t / n) M^2.  t = n / 5: 0.8 M^2, the tail is trimmed and the sites
    are proven as ever.  t = 3 n / 10: 1.2 M^2, nothing is trimmed, the centre follows the tail, every centred norm is of the
    order of M and no query can be proven -- the limit DESIGN.md states, from both sides."""
    ix = index("FloatEuclidian", 64, "clean", mu=4.0, centred=True, tail_share=share)
    st = ix.sites
    assert len(st.tail_pos) == st.n * share[0] // share[1] and (len(st.tail_pos) < st.n / 4) == (share == (1, 5))
    ix.run(monkeypatch, path, [SITE33, SITE65], rows=True)
    ctrs = ix.per_site(monkeypatch, path, [SITE33, SITE65])
    _note(f"centred mu=4, {len(st.tail_pos)} of {st.n} rows of norm 2^30 {path}: {_show(st, ctrs)}")
    if share == (1, 5):
        assert all(u <= REP // 10 for u, _ in ctrs.values()), ctrs
    else:
        assert all(u == REP for u, _ in ctrs.values()), ctrs


@pytest.mark.parametrize("path", PATHS)
def test_switch_order_on_one_index(index, oracle, wa, monkeypatch, path):
    """the two tables and the two centred buffers of an index are built at first use and chosen by the switches in force: flipped
    in an order in which the untrimmed buffer is built AFTER the trimmed one, every state's counters are those of an index that
    was put into that state directly"""
    kw = dict(mu=4.0)
    one = _Index(oracle, wa, "FloatEuclidian", 64, "outside", window_norms=False, **kw)
    sites = one.sites.sites_of(path)
    for step, state in enumerate(((True, False), (True, True), (False, True), (True, True), (True, False))):
        one.switch(*state)
        one.seen.clear()
        got = one.per_site(monkeypatch, path, sites)
        want = index("FloatEuclidian", 64, "outside", window_norms=state[0], centred=state[1], **kw).per_site(monkeypatch, path, sites)
        _note(f"switch order step {step + 1} window_norms={state[0]} centred={state[1]} {path}: {_show(one.sites, got)}")
        assert got == want, (step, state, got, want)


def test_tree_route(wa, gpu, monkeypatch, tmp_path):
    """the tree's exact-window route (test_gpu_dense_window_norms.test_tree_exact_windows' index): the outlier at label rank p, the
    last position of a block.  Windows that start AT p hold it: none is proven.  Windows that start at p + 1, a block boundary,
    have it one position outside their cover."""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    n, d, nq, k, L, p = 20000, 64, 64, 10, 16384, 5 * 2048 + 63
    rng = np.random.default_rng(11)
    X, labels = random_rows("FloatEuclidian", rng, n, d), rng.permutation(n).astype(np.float32)
    Q = random_rows("FloatEuclidian", rng, nq, d)
    # distinct widths; 32 windows end in the first 2 048-position block, 32 in the third: every block has its 32 queries
    w = np.concatenate([1100 + 25 * np.arange(32), 4100 + 59 * np.arange(32)])
    assert len(set(w.tolist())) == nq and w.min() >= 1100 and w.max() <= 6000 and p % 64 == 63
    X[np.nonzero(labels == p)[0][0]] *= np.float32(2.0 ** 30)
    idx = wa.VamanaRangeFilterTreeIndexFloatEuclidian(X, labels, cutoff=5000, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/"))
    idx.set_exact_windows(L)
    for a in (p, p + 1):
        got = {}
        for on in (False, True):
            assert idx.set_dense_window_norms(on) is on
            ids, dists = idx.batch_search(Q, pos_windows(a + 0 * w, a + w), nq, "optimized_postfilter", _qp(wa, k))
            got[on] = (ids, dists.view(np.uint32), idx.exact_window_counters())
            _note(f"tree, windows from p{'+1' if a > p else ''}, switch {on}: {got[on][2]}")
        assert np.array_equal(got[False][0], got[True][0]) and np.array_equal(got[False][1], got[True][1])
        on = got[True][2]
        assert on["queries"] == nq and on["dense_queries"] > 0, on
        if a == p:
            assert on["unproven"] == on["dense_queries"], on
        else:
            assert on["unproven"] <= nq // 10, on
