"""GPU: the centred dense path on float32 rows of 129 .. 512 elements (`set_dense_centred(True)` on the wide row class:
`k_gemm_scores_wide_centred<2|3|4>`, `k_row_centre` / `k_point_norms_centred` over up to 512 columns) -- test_gpu_dense_centred.py's
inputs, rows and queries mu 1 + unit noise, at the row lengths where the slab walk can go wrong: an almost-empty last slab (129),
two full slabs (256), three (300), zero columns inside the fourth (500), four full ones (512).  Every batch goes through
test_gpu_dense_numerics.py's three row checks (the same index's exact scan bit for bit, golden_util.same_rows against the oracle,
the float64 bounds); with the switch on at most a tenth of the queries may stay unproven, the cap those families keep at mu = 0
with the switch off, and with it off again more than that do."""
import numpy as np
import pytest

import numerics_util as nu
from test_gpu_dense_centred import _case, _queries_at_the_centre
from test_gpu_dense_numerics import PATHS, _run
from test_gpu_dense_window_norms import OUT_POS, _far_from_every_window

pytestmark = pytest.mark.gpu
CELLS = [(129, 4.0), (256, 4.0), (300, 4.0), (300, 1024.0), (500, 4.0), (512, 4.0), (512, 1024.0)]


def _capped(case, fam, path, k, tag):
    ctr = case.run(path, k)[2]
    print(f"[dense centred wide] {tag} {path} k={k}: {ctr}")
    assert ctr["unproven"] <= len(fam.Q) // 10, ctr


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("d,mu", CELLS)
def test_common_offset_is_proven(oracle, wa, gpu, monkeypatch, d, mu, path):
    fam, case = _case(oracle, wa, monkeypatch, "FloatEuclidian", d, mu)
    _capped(case, fam, path, 10, f"d={d} mu={mu:g}")
    if mu == 4.0:  # the switch alone moves the route: off again, the same batch on the same index is back at the uncentred bound
        assert case.pi.set_dense_centred(False) is False
        ctr = case.run(path, 10, rows=False)[2]
        print(f"[dense centred wide] d={d} mu={mu:g} {path} k=10 switch off: {ctr}")
        assert ctr["unproven"] > len(fam.Q) // 10, ctr


def test_large_k(oracle, wa, gpu, monkeypatch):
    """k = 17: k_large_rerank, whose windows need 96 x 17 positions (the cover path's narrowed windows fall short of that)"""
    fam, case = _case(oracle, wa, monkeypatch, "FloatEuclidian", 256, 4.0)
    assert (fam.b - fam.a).min() >= 1632 and case.pi.set_dense_large_k(True) is True
    _capped(case, fam, "shared", 17, "d=256 mu=4 large k")


def _outlier(fam, X, Q):
    X[fam.order[OUT_POS]] *= np.float32(2.0 ** 30)


@pytest.mark.parametrize("path", PATHS)
def test_outlier_and_window_norms(oracle, wa, gpu, monkeypatch, path):
    """with set_dense_window_norms as well: the trimmed centre over 256 columns and the table over its norms; the row of norm 2^30
    lies outside every window"""
    fam, case = _case(oracle, wa, monkeypatch, "FloatEuclidian", 256, 4.0, _outlier)
    _far_from_every_window(fam, OUT_POS)
    assert case.pi.set_dense_window_norms(True) is True
    _capped(case, fam, path, 10, "d=256 mu=4 outlier, window norms")


@pytest.mark.parametrize("path", PATHS)
def test_queries_at_the_centre(oracle, wa, gpu, monkeypatch, path):
    fam, case = _case(oracle, wa, monkeypatch, "FloatEuclidian", 300, 4.0, _queries_at_the_centre)
    print(f"[dense centred wide] queries at the centre d=300 {path}: {case.run(path, 10)[2]}")


@pytest.mark.parametrize("sfx", ("FloatMips", "Float16Euclidian"))
def test_other_routes_do_not_move(wa, gpu, monkeypatch, sfx):
    """inner product, and float16 rows of 256 elements (k_gemm_scores_hslab): switch on or off, the same rows and counters"""
    monkeypatch.setenv("WANN_DENSE_LONG_ROWS", "1")  # (the float16 rows take the dense path where the process opts in)
    fam = nu.Families(3256, 256, ["control"] * 6)
    elem = np.float16 if sfx.startswith("Float16") else np.float32
    X, Q = ((a.astype(np.float64) + 4.0).astype(elem) for a in (fam.X, fam.Q))
    pi = getattr(wa, "PrefilterIndex" + sfx)(X, fam.labels)
    got = []
    for on in (False, True):
        assert pi.set_dense_centred(on) is (on and sfx != "FloatMips")
        ids, dists, ctr = _run(pi, wa, monkeypatch, "shared", Q, fam.windows("shared"), 10)
        got.append((ids, dists.view(np.uint32), ctr))
    assert got[0][2] == got[1][2] and np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), got
