"""GPU: window maxima in the dense proof (`set_dense_window_norms(True)`: `k_norm_blocks`, `k_norm_levels`, `window_norm_max`).

test_gpu_dense_numerics.py's common-offset inputs at mu = 0 -- six control families, on which that file caps the unproven queries
at a tenth -- with ONE row scaled to a norm of 2^30 (float16: 2^15; float8: 64 times the others) at a position at least 256
positions from every window.  Without the switch the proof's bound is the outlier's and every query goes back to the scan; with
it the window maxima are those of the data without the outlier, so the same cap holds.  Every batch goes through that file's three
row checks (the same index's exact scan bit for bit, golden_util.same_rows against the oracle, the float64 bounds)."""
import numpy as np
import pytest

import numerics_util as nu
from test_gpu_dense_numerics import PATHS, _Case
from util import pos_windows, random_rows, wide_window_batch

pytestmark = pytest.mark.gpu
OUT_POS = nu.SLOT * 3 + 100
# d = 100: a padded row (112 floats); bfloat16 / float8: units of their own
CELLS = [("FloatEuclidian", 64), ("FloatMips", 100), ("Float16Euclidian", 100), ("BFloat16Euclidian", 64), ("Float8Euclidian", 64)]


class _UpcastOracle:
    """the float32 oracle under the bfloat16 / float8 class names: the rows passed are float32 values those types hold exactly"""

    def __init__(self, oracle):
        self._oracle = oracle

    def __getattr__(self, name):
        return getattr(self._oracle, name.replace("BFloat", "Float").replace("Float8", "Float"))


def _case(oracle, wa, monkeypatch, sfx, d, out_pos, mu=0.0):
    """the index over the control families with the row at position out_pos(fam) of the label order scaled up; switch on"""
    fam = nu.Families(3000 + d, d, ["control"] * 6)
    X, Q = ((a.astype(np.float64) + mu).astype(np.float32) for a in (fam.X, fam.Q))
    big = 2.0 ** (15 if sfx.startswith("Float16") else 30)
    if sfx.startswith("BFloat16"):
        X, Q = nu.bf16(X), nu.bf16(Q)
    if sfx.startswith("Float8"):  # (elements of about 8 / sqrt(d): E4M3's normal range; the outlier stays within 448)
        X, Q, big = wa.float8_round(X * np.float32(8)), wa.float8_round(Q * np.float32(8)), 64.0
    pos = out_pos(fam) if callable(out_pos) else out_pos
    X[fam.order[pos]] *= np.float32(big)
    assert np.abs(X[fam.order[pos]]).max() <= (448 if sfx.startswith("Float8") else 65504 if sfx.startswith("Float16") else np.inf)
    case = _Case(_UpcastOracle(oracle), wa, monkeypatch, sfx, fam, X, Q)
    assert case.pi.dense_window_norms() is False and case.pi.set_dense_window_norms(True) is True
    assert case.pi.counters()["dense_window_norms"] == 1
    return fam, case, pos


def _far_from_every_window(fam, pos):
    """at least 256 positions from every window's nearest edge: no rounding to 64 or 128 positions can pull it in"""
    assert (np.minimum(np.abs(fam.a - pos), np.abs(fam.b - 1 - pos)) >= 256).all() and not ((fam.a <= pos) & (pos < fam.b)).any()


def _on_then_off(case, fam, path, k, tag):
    cap = len(fam.Q) // 10
    ctr = case.run(path, k)[2]
    print(f"[dense window norms] {tag} {path} k={k} on: {ctr}")
    assert ctr["unproven"] <= cap, ctr
    assert case.pi.set_dense_window_norms(False) is False and case.pi.counters()["dense_window_norms"] == 0
    ctr = case.run(path, k, rows=False)[2]  # the same index and batch: the bound is the outlier's again
    print(f"[dense window norms] {tag} {path} k={k} off: {ctr} {case.pi.counters()}")
    assert ctr["unproven"] > cap, ctr
    assert case.pi.set_dense_window_norms(True) is True


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sfx,d", CELLS)
def test_outlier_outside_every_window(oracle, wa, gpu, monkeypatch, sfx, d, path):
    fam, case, pos = _case(oracle, wa, monkeypatch, sfx, d, OUT_POS)
    _far_from_every_window(fam, pos)
    _on_then_off(case, fam, path, 10, f"{sfx} d={d}")
    if (sfx, d, path) == ("FloatEuclidian", 64, "shared"):  # k = 17: rerank_query_large, whose windows need 96 x 17 positions
        assert (fam.b - fam.a).min() >= 1632 and case.pi.set_dense_large_k(True) is True
        _on_then_off(case, fam, path, 17, f"{sfx} d={d}")


@pytest.mark.parametrize("path", PATHS)
def test_outlier_and_common_offset(oracle, wa, gpu, monkeypatch, path):
    """with set_dense_centred as well, at mu = 4: the table over the centred norms -- and the trimmed centre (`k_norm_trim`,
    `k_row_centre_trimmed`): the mean of ALL rows would follow the 2^30 row by about 2^30 x 4 / n = 1.7e5 a column and make every
    centred norm that large (240 of 240 unproven, as measured before the centre was trimmed)"""
    fam, case, pos = _case(oracle, wa, monkeypatch, "FloatEuclidian", 64, OUT_POS, mu=4.0)
    _far_from_every_window(fam, pos)
    assert case.pi.set_dense_centred(True) is True
    _on_then_off(case, fam, path, 10, "FloatEuclidian d=64 centred mu=4")


@pytest.mark.parametrize("path", PATHS)
def test_outlier_inside_a_window(oracle, wa, gpu, monkeypatch, path):
    """the outlier at the LAST position of family 0's narrowest window: that family's bound must hold it (no query of it can be
    proven -- a block index one too low would prove them), the other five families never see it"""
    fam, case, pos = _case(oracle, wa, monkeypatch, "FloatEuclidian", 64, lambda fam: int(fam.positions(path)[1][:nu.REP].min()) - 1)
    own, others = np.arange(nu.REP), np.arange(nu.REP, len(fam.Q))
    a, b = fam.positions(path)
    assert ((a[own] <= pos) & (pos < b[own])).all() and not ((a[others] <= pos) & (pos < b[others])).any()
    c0, c1 = case.run(path, 10, own)[2], case.run(path, 10, others)[2]
    print(f"[dense window norms] inside window 0 {path}: its family {c0}, the others {c1}")
    assert c0["unproven"] == len(own), c0
    assert c1["unproven"] <= len(others) // 10, c1


def test_tree_exact_windows(wa, gpu, monkeypatch, tmp_path):
    """test_gpu_exact_windows.py's dense case (util.wide_window_batch, L = 16 384) at n = 20 000, with 512 more points at the end of
    the label order, the last of them the outlier: no window comes within 512 positions of it"""
    monkeypatch.delenv("WANN_NO_GEMM", raising=False)
    monkeypatch.setenv("WANN_DENSE_ALWAYS", "1")
    n0, n, d, nq, k, L = 20000, 20512, 64, 600, 10, 16384
    rng = np.random.default_rng(7)
    X, labels = random_rows("FloatEuclidian", rng, n, d), rng.permutation(n).astype(np.float32)
    Q = random_rows("FloatEuclidian", rng, nq, d)
    a, w = wide_window_batch(n0, nq, 70)
    assert (a + w).max() <= n - 1 - 256
    X[np.argmax(labels)] *= np.float32(2.0 ** 30)
    idx = wa.VamanaRangeFilterTreeIndexFloatEuclidian(X, labels, cutoff=5000, split_factor=2, build_params=wa.BuildParams(32, 64, 1.0, str(tmp_path) + "/"))
    idx.set_exact_windows(L)
    got = {}
    for on in (False, True):
        assert idx.set_dense_window_norms(on) is on
        ids, dists = idx.batch_search(Q, pos_windows(a, a + w), nq, "optimized_postfilter", wa.QueryParams(k, 10, 1.35, 10_000_000, 10_000, 1, 10000, None, False))
        got[on] = (ids, dists.view(np.uint32), idx.exact_window_counters())
        print(f"[dense window norms] tree switch {on}: {got[on][2]}")
    assert np.array_equal(got[False][0], got[True][0]) and np.array_equal(got[False][1], got[True][1])
    off, on = got[False][2], got[True][2]
    assert off["queries"] == on["queries"] == nq and off["dense_queries"] == on["dense_queries"] > nq // 2, (off, on)
    assert off["unproven"] == off["dense_queries"] and on["unproven"] <= nq // 10, (off, on)
