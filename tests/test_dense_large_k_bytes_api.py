"""CPU: the per-index switch of the byte units' large-k dense path (wann_set_dense_large_k_bytes; `k_large_rerank_b` /
`k_large_rerank_cover_b`) without a device: the C symbols on a null index, the kernels' register budget."""
import ctypes
import os
import subprocess
import sys

import pytest

from util import REPO


def test_a_null_index(wa):
    import rangefilteredann_amd
    lib = ctypes.CDLL(rangefilteredann_amd.lib_path())
    assert lib.wann_set_dense_large_k_bytes(None, 1) < 0 and lib.wann_set_dense_large_k_bytes(None, 0) < 0 and lib.wann_dense_large_k_bytes(None) == 0


@pytest.mark.parametrize("kernel", ("k_large_rerank_b", "k_large_rerank_cover_b"))
def test_library_holds_the_kernels_within_the_units_budget(wa, kernel):
    """both metrics x both key shifts in the uint8 and the int8 unit: at most 256 registers, no scratch, no spilled register"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), kernel + "I"], capture_output=True, text=True, timeout=300)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == 8 and sum("dt_u8" in l for l in lines) == 4 and sum("dt_i8" in l for l in lines) == 4, out.stdout + out.stderr
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256 and int(l.split("scratch")[1].split()[0]) == 0 and int(l.split(" spill")[1].split()[0]) == 0, l
