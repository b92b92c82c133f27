"""CPU: what of the long-row dense path for byte rows (uint8 / int8 rows of 513 .. 2048 bytes, `k_gemm_scores_bslab`) shows without
a device: the built library holds the score kernel once per byte unit, within the register budget of two waves per SIMD and
without a scratch segment, and the documents name the limit beside the switch that opts in to it."""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _resources(name):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), name], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return [l for l in out.stdout.splitlines() if name in l]


def test_library_holds_the_byte_slab_kernel_without_scratch(wa):
    lines = _resources("k_gemm_scores_bslab")
    assert len(lines) == 2 and any("dt_u8" in l for l in lines) and any("dt_i8" in l for l in lines), lines  # (the byte units only)
    for l in lines:
        regs = int(l.split("vgpr+agpr")[1].split()[0])
        scratch = int(l.split("scratch")[1].split()[0])
        spill = int(l.split(" spill")[1].split()[0])
        assert regs <= 512 and scratch == 0 and spill == 0, l
        assert regs <= 256, l  # two workgroups share a CU (two waves per SIMD): the launcher's grid and DESIGN.md 3.5 assume it
    assert len(_resources("k_pack_queries_b")) == 2
    # the names the float32 test counts stay its own
    assert not any("k_gemm_scores_long" in l or "k_split_queries" in l for l in lines + _resources("k_pack_queries_b"))


def test_documents_name_the_limit():
    assert re.search(r"uint8 / int8 rows of up to 2048 bytes", _read(REPO, "README.md"))
    assert re.search(r"uint8 / int8 rows of at most 2048 bytes", _read(REPO, "INTEGRATION.md"))
    design = _read(REPO, "DESIGN.md")
    assert "k_gemm_scores_bslab" in design and re.search(r"uint8 / int8 rows are done up to 2048 bytes", design)
    header = _read(REPO, "include", "wann.h")
    assert "2048 bytes" in header and "WANN_DENSE_LONG_ROWS" in header
    # rows of more than 512 bytes are opt-in: every document states the limit in a paragraph that names the switch
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        paras = [p for p in re.split(r"\n\s*\n", _read(REPO, doc)) if "2048 bytes" in p]
        assert paras and any("WANN_DENSE_LONG_ROWS" in p for p in paras), doc
