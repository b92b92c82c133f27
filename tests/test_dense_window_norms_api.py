"""CPU: what of wann_set_dense_window_norms shows without a device: the two C symbols, their answers on a null index, and the
table kernels -- `k_norm_blocks` and `k_norm_levels` in each of the four float units, without scratch or spills."""
import ctypes
import os
import subprocess
import sys

import pytest

from util import REPO


def test_symbols_and_a_null_index(wa):
    import rangefilteredann_amd
    lib = ctypes.CDLL(rangefilteredann_amd.lib_path())
    header = open(os.path.join(REPO, "include", "wann.h")).read()
    assert "int wann_set_dense_window_norms(wann_index *index, int on);" in header and "int wann_dense_window_norms(const wann_index *index);" in header
    assert lib.wann_set_dense_window_norms(None, 1) < 0 and lib.wann_set_dense_window_norms(None, 0) < 0 and lib.wann_dense_window_norms(None) == 0
    assert lib.wann_abi_version() == 5


def test_table_kernels_in_every_float_unit(wa):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_norm_"], capture_output=True, text=True, timeout=300)
    if out.returncode != 0 or not out.stdout.strip():
        pytest.skip("ROCm llvm tools not present")
    lines = out.stdout.splitlines()
    for kern in ("13k_norm_blocksE", "13k_norm_levelsE"):
        for unit in ("_ZN4wann", "_ZN4wann6dt_f16", "_ZN4wann7dt_bf16", "_ZN4wann5dt_f8"):  # float32 (no unit namespace), float16, bfloat16, float8
            assert sum(l.startswith(unit + kern) for l in lines) == 1, (unit, kern, lines)
    assert len(lines) == 8 + 2, lines  # (and in no byte unit; + k_norm_trim of the float32 and float16 units: the trimmed centre)
    assert sum("11k_norm_trimE" in l for l in lines) == 2, lines
    for l in lines:
        assert int(l.split("scratch")[1].split()[0]) == 0 and int(l.split(" spill")[1].split()[0]) == 0, l
