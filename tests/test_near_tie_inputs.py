"""CPU: the near-tie inputs of tests/test_gpu_dense_numerics.py really are inputs on which the split-bf16 score order and the
exact distance order disagree.  Checked with the numpy model of the score arithmetic (numerics_util) and float64 distances, for
the seeds the GPU tests use.  The shares are conditions on the INPUTS (measured when they were designed: 36 - 38 of 50 queries
under L2, 6 - 14 of 50 under the inner product at sigma = 2^-20, none at 2^-17), not measurements of any kernel."""
import numpy as np
import pytest

import numerics_util as nu


def test_bf16_rounds_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.14159274, 2.0 ** -100, 0.0], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625, 2.0 ** -100, 0.0], dtype=np.float32)
    assert np.array_equal(nu.bf16(x), want)
    rng = np.random.default_rng(0)
    y = (rng.standard_normal(10000) * 2.0 ** rng.integers(-60, 60, 10000)).astype(np.float32)
    hi, lo = nu.split(y)
    assert (np.abs(y.astype(np.float64) - hi - lo.astype(np.float64)) <= 2.0 ** -16 * np.abs(y)).all()
    assert (np.abs(y.astype(np.float64) - hi) <= 2.0 ** -8 * np.abs(y)).all()


@pytest.mark.parametrize("sfx,d", nu.NEAR_TIE_CASES)
def test_shells_defeat_the_score_order(sfx, d):
    fam = nu.near_tie_families(d)
    metric = "mips" if sfx.endswith("Mips") else "l2"
    shell = fam.is_shell
    assert shell.sum() == 8 * nu.REP and (~shell).sum() == 4 * nu.REP
    for f, pos in fam.shell_pos.items():  # every shell lies inside every window of its family, on both paths
        assert len(pos) >= 128 and pos.min() >= fam.a[f] + nu.REP - 1 and pos.max() < fam.b[f] - nu.REP + 1
        step = np.unique(pos // 128)
        assert len(step) <= 2 if fam.kind[f] == "contiguous" else len(step) >= 10
    for k in (1, 10, 16):
        out = fam.outside_keep(metric, k)
        print(f"[near-tie inputs] {sfx} d={d} k={k}: top k outside the {nu.KEEP} best scores for {int(out[shell].sum())} of "
              f"{int(shell.sum())} shell queries, {int(out[~shell].sum())} of {int((~shell).sum())} control queries")
        if k == 10:
            assert out[shell].sum() * (10 if metric == "mips" else 2) >= shell.sum(), (k, int(out[shell].sum()))
        assert not out[~shell].any()  # the control queries' rows are well spread: the scores settle them


@pytest.mark.parametrize("metric", ("l2", "mips"))
def test_ladder_shells_bite_and_stay_normal(metric):
    """the scale ladder's grid inputs: they bite at k = 10 as well, and on the grid every product term q_i p_i and every
    difference q_i - p_i inside a window is zero or large enough (2^-18, 2^-12) to stay normal in fp32 at a joint scale of 2^-100"""
    fam = nu.ladder_families("shell")
    out = fam.outside_keep(metric, 10)
    shell = fam.is_shell
    print(f"[near-tie inputs] ladder {metric}: {int(out[shell].sum())} of {int(shell.sum())}")
    assert out[shell].sum() * (10 if metric == "mips" else 2) >= shell.sum()
    for f in range(fam.F):
        P = fam.X[fam.window_rows(f)].astype(np.float64)
        for q in fam.Q[f * nu.REP:(f + 1) * nu.REP].astype(np.float64):
            prod, diff = np.abs(P * q), np.abs(P - q)
            assert prod[prod > 0].min() >= 2.0 ** -18.01 and diff[diff > 0].min() >= 2.0 ** -12.01
