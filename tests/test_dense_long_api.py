"""CPU: what of the long-row dense path (float32 rows of 513 .. 2048 floats, `k_gemm_scores_long`) shows without a device: the
built library holds the two kernels, the score kernel within its register budget and without a scratch segment, and the documents
name the limit and the switch that opts in to it."""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_library_holds_the_long_row_kernels_without_scratch(wa):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_gemm_scores_long"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if "k_gemm_scores_long" in l]
    assert len(lines) == 1, out.stdout  # (float32 unit only)
    regs = int(lines[0].split("vgpr+agpr")[1].split()[0])
    scratch = int(lines[0].split("scratch")[1].split()[0])
    spill = int(lines[0].split(" spill")[1].split()[0])
    assert regs <= 512 and scratch == 0 and spill == 0, lines[0]  # one wave per SIMD: 512 registers; nothing in memory
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_split_queries"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and len([l for l in out.stdout.splitlines() if "k_split_queries" in l]) == 1, out.stdout


def test_documents_name_the_limit():
    assert re.search(r"float32 rows of up to 2048 elements", _read(REPO, "README.md"))
    assert re.search(r"float32 rows of at most 2048 dimensions", _read(REPO, "INTEGRATION.md"))
    design = _read(REPO, "DESIGN.md")
    assert "k_gemm_scores_long" in design and re.search(r"float32 rows are done up to 2048 floats", design)
    # rows of more than 512 floats are opt-in: every document that states the limit names the switch
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "WANN_DENSE_LONG_ROWS" in _read(REPO, doc), doc
