"""CPU: the oracle against the REAL reference.  Where a reference build is present (oracle/_ref, `make -C oracle ref`) the two
run side by side on the same graph files.  Everywhere else the oracle builds the graphs itself and its graph files and rows are
checked against the SHA-256 digests of what the reference wrote and returned for the same inputs
(tests/golden/oracle_vs_reference.json, written by tests/golden/make_oracle_vs_reference_golden.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

import golden_util as gu
from util import REPO, distinct_labels, quiet_stdout, repeated_labels, sift_like, tie_heavy, tie_queries, tie_windows, unit_mixture, windows

GOLDEN = os.path.join(REPO, "tests", "golden", "oracle_vs_reference.json")


def digest(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a).astype(dtype)).tobytes()).hexdigest()


def row_digests(ids, dists):
    return {"ids": digest(ids, np.int64), "dists": digest(dists, np.float32)}


def file_digests(path):
    return {f: hashlib.sha256(open(os.path.join(path, f), "rb").read()).hexdigest() for f in sorted(os.listdir(path))}


@pytest.fixture(scope="module")
def ref(oracle):
    """the reference's module, or None: replay the stored digests"""
    os.environ.setdefault("PARLAY_NUM_THREADS", "4")
    return oracle.load_reference()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


KINDS = ["VamanaRangeFilterTreeIndex", "SuperOptimizedPostfilterTreeIndex", "PostfilterVamanaIndex", "RangeFilterTreeIndex", "PrefilterIndex"]
EQUALS_CASES = [("Euclidian", sift_like, 128), ("mips", unit_mixture, 100), ("Euclidian", unit_mixture, 104)]
RATIO_CASES = [("Euclidian", sift_like, 64), ("mips", unit_mixture, 100)]
BUILDER_CASES = [("Euclidian", 1500, 16, 16, 40), ("mips", 3000, 24, 12, 32), ("Euclidian", 9000, 16, 8, 20)]


def equals_key(kind, metric, gen, d):
    return f"equals|{kind}|{metric}|{gen.__name__}|{d}"


def equals_rows(mod, cache, kind, metric, gen, d):
    """`mod`'s index of the case on the graph files under `cache` (built there when absent) and its rows: {case: (ids, dists)}"""
    n, nq = 2500, 60
    g = gen(n, d, 31)
    X, Q = g(n), g(nq)
    labels = distinct_labels(n, 12)
    sfx = "FloatMips" if metric == "mips" else "FloatEuclidian"
    kw = dict(cutoff=250, split_factor=2) if "Tree" in kind else {}
    if kind.startswith("Super"):
        kw["shift_factor"] = 0.5
    labkw = "filters" if kind == "PostfilterVamanaIndex" else "filter_values"
    with quiet_stdout():
        idx = getattr(mod, kind + sfx)(X, **{labkw: labels}, build_params=mod.BuildParams(24, 48, 1.0, cache), **kw)
    methods = ["optimized_postfilter", "fenwick", "three_split"] if kind.endswith("RangeFilterTreeIndex") else [None]
    rows = {}
    for p in (-5, -3, -1, 0):
        W = windows(labels, nq, p, 40 + p)
        for method in methods:
            for beam, mult in [(10, 1), (40, 2)]:
                a = (Q, W, nq) + ((method,) if method else ())
                with quiet_stdout():
                    rows[f"{p}|{method}|{beam}|{mult}"] = idx.batch_search(*a, mod.QueryParams(10, beam, 1.35, 10**7, 10**4, mult, 10000, None, False))
    return rows


@pytest.mark.parametrize("metric,gen,d", EQUALS_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_reference(oracle, ref, golden, tmp_path, metric, gen, d, kind):
    cache = str(tmp_path) + "/"
    want = None
    if ref is not None:  # the reference builds and writes the graph cache; the oracle loads it
        want = equals_rows(ref, cache, kind, metric, gen, d)
    got = equals_rows(oracle, cache, kind, metric, gen, d)
    g = golden[equals_key(kind, metric, gen, d)]
    if ref is None:  # the oracle built the graphs: the reference's files, byte for byte
        assert file_digests(cache) == g["graphs"]
    integer_data = gen is sift_like
    check_ids = not integer_data or kind in ("SuperOptimizedPostfilterTreeIndex", "PostfilterVamanaIndex")
    for case, (oi, od) in got.items():
        ids_too = check_ids or (kind == "VamanaRangeFilterTreeIndex" and case.split("|")[1] == "optimized_postfilter")
        if want is not None:
            ri, rd = want[case]
            assert np.array_equal(rd, od), (kind, case)
            if ids_too:
                assert np.array_equal(ri, oi), (kind, case)
        else:
            assert row_digests(oi, od)["dists"] == g["rows"][case]["dists"], (kind, case)
            if ids_too:
                assert row_digests(oi, od)["ids"] == g["rows"][case]["ids"], (kind, case)


def ratio_key(metric, gen, d):
    return f"ratio|{metric}|{gen.__name__}|{d}"


def ratio_rows(mod, cache, metric, gen, d):
    n, nq = 2500, 60
    g = gen(n, d, 77)
    X, Q = g(n), g(nq)
    labels = distinct_labels(n, 13)
    sfx = "FloatMips" if metric == "mips" else "FloatEuclidian"
    with quiet_stdout():
        idx = getattr(mod, "VamanaRangeFilterTreeIndex" + sfx)(X, filter_values=labels, cutoff=250, split_factor=2,
                                                                   build_params=mod.BuildParams(24, 48, 1.0, cache))
    rows = {}
    for p in (-5, -3, -1):
        W = windows(labels, nq, p, 90 + p)
        for ratio in (None, 1.0, 1.5, 3.0, 8.0):
            for beam, mult in [(10, 1), (40, 2)]:
                with quiet_stdout():
                    rows[f"{p}|{ratio}|{beam}|{mult}"] = idx.batch_search(Q, W, nq, "optimized_postfilter",
                                                                          mod.QueryParams(10, beam, 1.35, 10**7, 10**4, mult, 10000, ratio, False))
    return rows


@pytest.mark.parametrize("metric,gen,d", RATIO_CASES)
def test_oracle_ratio_fallback_equals_reference(oracle, ref, golden, tmp_path, metric, gen, d):
    """min_query_to_bucket_ratio (src/range_filter_tree.h:460-466): windows that are a small share of their smallest containing
    bucket take fenwick_tree_search -- distances identical for every ratio, ids wherever no merged list is involved"""
    cache = str(tmp_path) + "/"
    want = ratio_rows(ref, cache, metric, gen, d) if ref is not None else None
    got = ratio_rows(oracle, cache, metric, gen, d)
    g = golden[ratio_key(metric, gen, d)]
    if ref is None:
        assert file_digests(cache) == g["graphs"]
    changed = 0
    for case, (oi, od) in got.items():
        if want is not None:
            ri, rd = want[case]
            assert np.array_equal(rd, od), case
            if gen is not sift_like:  # (integer data: merged lists hold distance ties the reference orders arbitrarily)
                assert np.array_equal(ri, oi), case
        else:
            assert row_digests(oi, od)["dists"] == g["rows"][case]["dists"], case
            if gen is not sift_like:
                assert row_digests(oi, od)["ids"] == g["rows"][case]["ids"], case
        p, ratio, beam, mult = case.split("|")
        if ratio != "None" and (beam, mult) == ("40", "2") and not np.array_equal(got[f"{p}|None|40|2"][1], od):
            changed += 1
    assert changed > 0  # some ratio did send queries down the other branch


def builder_key(metric, n, d, R, L):
    return f"builder|{metric}|{n}|{d}|{R}|{L}"


def builder_files(mod, cache, metric, n, d, R, L):
    rng = np.random.default_rng(n + d)
    X = rng.standard_normal((n, d)).astype(np.float32)
    if metric == "mips":
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    labels = distinct_labels(n, 3)
    sfx = "FloatMips" if metric == "mips" else "FloatEuclidian"
    os.makedirs(cache)
    with quiet_stdout():
        getattr(mod, "VamanaRangeFilterTreeIndex" + sfx)(X, filter_values=labels, cutoff=400, split_factor=2, build_params=mod.BuildParams(R, L, 1.0, cache))
    return file_digests(cache)


@pytest.mark.parametrize("metric,n,d,R,L", BUILDER_CASES)  # L2: d % 8 == 0 (the reference reads past d otherwise)
def test_oracle_builder_equals_reference_builder(oracle, ref, golden, tmp_path, metric, n, d, R, L):
    """Whole tree of graphs (every partition size down to the leaves) on continuous coordinates: every cache
    file the oracle's builder writes equals the reference builder's.  (With exactly equidistant candidates
    the reference's result depends on libstdc++'s std::sort tie order -- vamana/index.h:77-78, graph.h:106 --
    and the restatement breaks such ties by id instead)"""
    want = builder_files(ref, str(tmp_path / "ref") + "/", metric, n, d, R, L) if ref is not None else golden[builder_key(metric, n, d, R, L)]
    got = builder_files(oracle, str(tmp_path / "orc") + "/", metric, n, d, R, L)
    assert sorted(got) == sorted(want) and len(got) > 3
    differing = [f for f in want if got[f] != want[f]]
    assert not differing, differing


# ------------------------------------------------------------------------------------------
# tie-heavy rows: d = 6 small integers, 15 % duplicated rows -- most distances are shared by many points
# ------------------------------------------------------------------------------------------
FLT_MAX = np.finfo(np.float32).max
TIE_CASES = [(kind, sfx, "distinct") for sfx in ("FloatEuclidian", "UInt8Euclidian") for kind in KINDS] + \
            [("PrefilterIndex", sfx, "repeated") for sfx in ("FloatEuclidian", "UInt8Euclidian")]


def ties_key(kind, sfx, labs):
    return f"ties|{kind}|{sfx}|{labs}"


def ties_rows(mod, cache, kind, sfx, labs):
    """`mod`'s index of the case, built on the graph files under `cache` (written there when absent), and its rows with the
    inputs they came from: {case: (ids, dists, W, method)}"""
    n, nq = 2500, 60
    d = 8 if sfx.startswith("Float") else 6  # (float32 L2: d % 8 == 0, the reference reads past d otherwise)
    X = tie_heavy(n, d, 17)
    Q = tie_queries(X, nq, 18)
    labels = distinct_labels(n, 12) if labs == "distinct" else repeated_labels(n, 12, 40)
    kw = dict(cutoff=250, split_factor=2) if "Tree" in kind else {}
    if kind.startswith("Super"):
        kw["shift_factor"] = 0.5
    labkw = "filters" if kind == "PostfilterVamanaIndex" else "filter_values"
    with quiet_stdout():
        idx = getattr(mod, kind + sfx)(X, **{labkw: labels}, build_params=mod.BuildParams(24, 48, 1.0, cache), **kw)
    methods = ["optimized_postfilter", "fenwick", "three_split"] if kind.endswith("RangeFilterTreeIndex") else [None]
    rows = {}
    for p in (-7, -5, -3, -1):
        W = tie_windows(labels, nq, p, 20 + p)
        for method in methods:
            for beam, mult in [(10, 1), (40, 2)]:
                a = (Q, W, nq) + ((method,) if method else ())
                with quiet_stdout():
                    ids, dists = idx.batch_search(*a, mod.QueryParams(10, beam, 1.35, 10**7, 10**4, mult, 10000, None, False))
                rows[f"{p}|{method}|{beam}|{mult}"] = (ids, dists, W, method)
    return X, labels, Q, rows


def prefilter_counts(labels, W, k):
    """rows a PrefilterIndex returns per window: positions [lower_bound(lo), lower_bound(hi)), both clipped to n - 1
    (prefiltering.h:159-184); the reference reads past the end of shorter lists, so only these entries are defined"""
    s = np.sort(np.asarray(labels, dtype=np.float32))
    lo, hi = np.asarray(W, dtype=np.float64).astype(np.float32).T
    a = np.minimum(np.searchsorted(s, lo, "left"), len(s) - 1)
    b = np.minimum(np.searchsorted(s, hi, "left"), len(s) - 1)
    return np.clip(b.astype(np.int64) - a, 0, k)


def canonical_rows(kind, ids, dists, labels, W, method):
    """The rows with what the reference leaves open replaced by what it does not: undefined padding -> (-1, FLT_MAX); in rows
    answered by an exact scan or a merged list (gu.exact_rows: an unstable sort-by-distance) the ids of each run of equal
    distances sorted, and those of a run that reaches the k boundary -- part of a larger tie group -- replaced by -2."""
    ids, dists = np.asarray(ids).astype(np.int64), np.array(dists, dtype=np.float32)
    k = ids.shape[1]
    if kind == "PrefilterIndex":
        cnt = prefilter_counts(labels, W, k)
        pad = np.arange(k)[None, :] >= cnt[:, None]
        ids[pad], dists[pad] = -1, FLT_MAX
    for r in np.flatnonzero(gu.exact_rows(kind, method, labels, W, 250)):
        j = 0
        while j < k:
            e = j
            while e + 1 < k and dists[r, e + 1] == dists[r, j]:
                e += 1
            ids[r, j:e + 1] = -2 if (e == k - 1 and dists[r, j] != FLT_MAX) else np.sort(ids[r, j:e + 1])
            j = e + 1
    return ids, dists


@pytest.mark.parametrize("kind,sfx,labs", TIE_CASES)
def test_oracle_equals_reference_on_tie_heavy_rows(oracle, ref, golden, tmp_path, kind, sfx, labs):
    """Small integer rows (d = 8 float32, d = 6 uint8, values 0..11), with distinct labels for every kind: both builders break distance ties the same
    way, so the graph files are byte-equal and the rows of a single beam search exact; rows that the reference answers with an
    exact scan or a merged list are equal up to the order of equal distances.  Repeated labels (40 values, runs of about 60
    points) for PrefilterIndex only: which points a window selects does not depend on how the reference's unstable
    parlay::sort_inplace orders equal labels, its rows up to ties do not either.  The tree kinds cannot be held to the reference
    on repeated labels -- its unstable label sort (tree_utils.h:68-73) changes which points each partition holds -- the GPU
    tests (tests/test_gpu_ties.py) check them against the oracle, which sorts stably by (label, id) as the product does."""
    co = str(tmp_path / "orc") + "/"
    os.makedirs(co)
    X, labels, Q, got = ties_rows(oracle, co, kind, sfx, labs)
    g = golden.get(ties_key(kind, sfx, labs)) if ref is not None else golden[ties_key(kind, sfx, labs)]
    if ref is not None:  # both build their own graphs: byte for byte the same files
        cr = str(tmp_path / "ref") + "/"
        os.makedirs(cr)
        want = ties_rows(ref, cr, kind, sfx, labs)[3]
        assert file_digests(co) == file_digests(cr)
    else:
        assert file_digests(co) == g["graphs"]
    metric = gu.metric_of(sfx)
    if kind == "RangeFilterTreeIndex":  # (the exact window rule of this kind: the oracle's own candidates, gu.window_rule)
        with quiet_stdout():
            cand_index = getattr(oracle, kind + sfx)(X, filter_values=labels, cutoff=250, split_factor=2,
                                                     build_params=oracle.BuildParams(24, 48, 1.0, co))
    for case, (oi, od, W, method) in got.items():
        ci, cd = canonical_rows(kind, oi, od, labels, W, method)
        if ref is not None:
            ri, rd, _, _ = want[case]
            cri, crd = canonical_rows(kind, ri, rd, labels, W, method)
            assert np.array_equal(crd, cd) and np.array_equal(cri, ci), (kind, case)
            rule = gu.window_rule(kind, method)
            beam, mult = (int(x) for x in case.split("|")[2:])
            cands = None
            if rule == "candidates":
                cands = gu.oracle_candidates(cand_index, Q, W, method,
                                             lambda k: oracle.QueryParams(k, beam, 1.35, 10**7, 10**4, mult, 10000, None, False))
            ctx = gu.RowContext(X, labels, Q, W, metric, rule, cands)
            ok, why = gu.same_rows(np.where(cri == -1, oi, ri), crd, oi, cd, gu.exact_rows(kind, method, labels, W, 250), ctx)
            assert ok, (kind, case, why)
        else:
            assert row_digests(ci, cd) == g["rows"][case], (kind, case)
