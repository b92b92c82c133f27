"""GPU: the centred dense path (`set_dense_centred(True)`: `k_row_centre`, `k_point_norms_centred`, `k_gemm_scores<STRIDE, true>`
and the proof on centred norms) on rows and queries mu 1 + unit noise -- test_gpu_dense_numerics.py's common-offset inputs, which
without the switch send every query back to the scan from mu = 4 on.  Every batch goes through that file's three row checks (the
same index's exact scan bit for bit, golden_util.same_rows against the oracle, the float64 bounds of its docstring) and counts
every query on its path; with the switch on at most a tenth may stay unproven, the cap that file applies at mu = 0: the centred
norms lie within 1 % of the norms at mu = 0."""
import numpy as np
import pytest

import numerics_util as nu
from test_gpu_dense_numerics import PATHS, _Case, _run

pytestmark = pytest.mark.gpu
# d = 100 is a row of 112 floats (padding columns); float16 stops at mu = 4: at 1024 a half's spacing is 1 and the noise is gone
CELLS = [("FloatEuclidian", 64, 4.0), ("FloatEuclidian", 64, 1024.0), ("FloatEuclidian", 100, 4.0), ("FloatEuclidian", 100, 1024.0),
         ("Float16Euclidian", 100, 4.0)]


def _case(oracle, wa, monkeypatch, sfx, d, mu, edit=None):
    fam = nu.Families(3000 + d, d, ["control"] * 6)
    X, Q = ((a.astype(np.float64) + mu).astype(np.float32) for a in (fam.X, fam.Q))
    if edit is not None:
        edit(fam, X, Q)
    case = _Case(oracle, wa, monkeypatch, sfx, fam, X, Q)
    assert case.pi.dense_centred() is False and case.pi.set_dense_centred(True) is True and case.pi.counters()["dense_centred"] == 1
    return fam, case


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sfx,d,mu", CELLS)
def test_common_offset_is_proven(oracle, wa, gpu, monkeypatch, sfx, d, mu, path):
    fam, case = _case(oracle, wa, monkeypatch, sfx, d, mu)
    cap = len(fam.Q) // 10
    for k in (10, 16) if (sfx, d, mu) == ("FloatEuclidian", 100, 4.0) else (10,):
        ctr = case.run(path, k)[2]
        print(f"[dense centred] {sfx} d={d} {path} mu={mu:g} k={k}: {ctr}")
        assert ctr["unproven"] <= cap, ctr
    if (sfx, d, mu, path) == ("FloatEuclidian", 64, 4.0, "shared"):  # k = 17: k_large_rerank, whose windows need 96 x 17 positions
        assert (fam.b - fam.a).min() >= 1632 and case.pi.set_dense_large_k(True) is True
        ctr = case.run(path, 17)[2]
        print(f"[dense centred] {sfx} d={d} {path} mu={mu:g} k=17: {ctr}")
        assert ctr["unproven"] <= cap, ctr
    if mu == 4.0:  # the switch alone moves the route: off again, the same batch on the same index has every query unproven, as before
        assert case.pi.set_dense_centred(False) is False
        ctr = case.run(path, 10, rows=False)[2]
        print(f"[dense centred] {sfx} d={d} {path} mu={mu:g} k=10 switch off: {ctr}")
        assert ctr["unproven"] == len(fam.Q), ctr


def _one_vector(fam, X, Q):
    X[fam.window_rows(0)] = X[fam.window_rows(0)[0]]  # family 0: every distance of a query ties, only the scan's id order settles it


def _queries_at_the_centre(fam, X, Q):
    Q[::8] = X.astype(np.float64).mean(axis=0).astype(np.float32)  # |fl(q - c)|^2 is rounding residue: E sits near its floor


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("edit", (_one_vector, _queries_at_the_centre))
def test_degenerate_rows_and_queries(oracle, wa, gpu, monkeypatch, edit, path):
    fam, case = _case(oracle, wa, monkeypatch, "FloatEuclidian", 64, 4.0, edit)
    print(f"[dense centred] {edit.__name__} {path}: {case.run(path, 10)[2]}")


def test_dense_rows_keeps_precedence(wa, gpu, monkeypatch):
    """integers 0 .. 255 with set_dense_rows(True): the score launches read the one-byte copy, centred switch on or off -- the same
    rows, the same counters"""
    fam = nu.Families(3064, 64, ["control"] * 6)
    rng = np.random.default_rng(64)
    X, Q = (rng.integers(0, 256, a.shape).astype(np.float32) for a in (fam.X, fam.Q))
    pi = wa.PrefilterIndexFloatEuclidian(X, fam.labels)
    assert pi.set_dense_rows(True) is True
    got = []
    for on in (False, True):
        assert pi.set_dense_centred(on) is on
        ids, dists, ctr = _run(pi, wa, monkeypatch, "shared", Q, fam.windows("shared"), 10)
        got.append((ids, dists.view(np.uint32), ctr, pi.counters()["dense_rows"]))
    assert got[0][3] == 1 and got[0][2:] == got[1][2:] and np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), got
