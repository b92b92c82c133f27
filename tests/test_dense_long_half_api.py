"""CPU: what of the float16 long-row dense path (rows of 129 .. 2048 elements, `k_gemm_scores_hslab`) shows without a device: the
built library holds the kernel once, in the float16 unit, within its register budget and without a scratch segment; the documents
name the limit and the switch that opts in to it; and the batches of tests/test_gpu_dense_long_half.py stay inside that test's
cap on unproven queries by the score model alone."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_long_half_inputs as inp
import numerics_util as nu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_library_holds_the_half_row_kernel_without_scratch(wa):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_gemm_scores_hslab"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if "k_gemm_scores_hslab" in l]
    assert len(lines) == 1 and "dt_f16" in lines[0], out.stdout  # (float16 unit only)
    # a name of its own: tests/test_dense_long_api.py counts the float32 kernels by name
    assert "k_gemm_scores_long" not in lines[0] and "k_split_queries" not in lines[0], lines[0]
    regs = int(lines[0].split("vgpr+agpr")[1].split()[0])
    scratch = int(lines[0].split("scratch")[1].split()[0])
    spill = int(lines[0].split(" spill")[1].split()[0])
    assert regs <= 512 and scratch == 0 and spill == 0, lines[0]  # one wave per SIMD: 512 registers; nothing in memory


def test_documents_name_the_limit_and_the_switch():
    paras = [p for p in re.split(r"\n\s*\n", _read(REPO, "README.md")) if "float16 rows of up to 2048 elements" in p]
    assert paras and all("WANN_DENSE_LONG_ROWS" in p for p in paras), paras
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = _read(REPO, doc)
        assert "k_gemm_scores_hslab" in text and "WANN_DENSE_LONG_ROWS" in text, doc


def _model_unprovable(bt, metric, k):
    """Queries of the batch whose top k the score model cannot prove: d_k + E >= cut - E, where d_k is the k-th float64 distance in
    the query's window, cut the worst of k_rerank's 32 candidates when they are the 32 best scores of the window (what the blocks
    hand over can only be worse; L2 scores get |q|^2 back), and E k_rerank's bound with the true d:
    c = 3.02 2^-16 + 3 (3 d + 8) 2^-24 + 2^-17, E = c |q| pmax under the inner product and 2 c (|q|^2 + pmax^2) under L2 -- for
    these unit rows four times c |q| pmax, the stricter of the two readings."""
    X, Q = bt.X32, bt.Q32
    c = 3.02 * 2.0 ** -16 + 3.0 * (3 * bt.d + 8) * 2.0 ** -24 + 2.0 ** -17
    p2max = float((X.astype(np.float64) ** 2).sum(axis=1).astype(np.float32).max())
    bad = 0
    for f in range(inp.F):
        rows = bt.order[bt.a[f]:bt.b[f]]
        q = Q[bt.family == f]
        sc = nu.emulated_scores(X[rows], q, metric)
        dd = nu.dist64(X[rows], q, metric)
        q2 = (q.astype(np.float64) ** 2).sum(axis=1)
        E = c * np.sqrt(q2 * p2max) if metric == "mips" else 2.0 * c * (q2 + p2max)
        dk = np.sort(dd, axis=1)[:, k - 1]
        cut = np.sort(sc, axis=1)[:, nu.KEEP - 1] + (0.0 if metric == "mips" else q2)
        bad += int((dk + E >= cut - E).sum())
    return bad


@pytest.mark.parametrize("d", inp.DIMS)
def test_batches_stay_inside_the_cap_by_the_model(d):
    """the GPU test's cap (a tenth of the batch unproven) is within reach of a correct kernel on every batch it runs: the inputs
    alone do not exceed it"""
    bt = inp.Batch(d)
    for metric in ("l2", "mips"):
        for k in sorted({k for dd, k in inp.SHARED_CASES if dd == d}):
            bad = _model_unprovable(bt, metric, k)
            print(f"[dense long half model] d={d} {metric} k={k}: {bad} of {len(bt.Q)} queries cannot be proven")
            assert bad <= len(bt.Q) // 10, (d, metric, k, bad)
