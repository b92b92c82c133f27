"""CPU: what of the centred dense path (wann_set_dense_centred; `k_gemm_scores<STRIDE, true>`) shows without a device: the two C
symbols, their answers on a null index, and the register budget of the score kernels -- the centred instances within two workgroups
per CU and without scratch, the uncentred ones at the parent build's figures (profiles/dense_centred_kernel_resources.txt)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from util import REPO


def test_symbols_and_a_null_index(wa):
    import rangefilteredann_amd
    lib = ctypes.CDLL(rangefilteredann_amd.lib_path())
    header = open(os.path.join(REPO, "include", "wann.h")).read()
    assert "int wann_set_dense_centred(wann_index *index, int on);" in header and "int wann_dense_centred(const wann_index *index);" in header
    assert lib.wann_set_dense_centred(None, 1) < 0 and lib.wann_set_dense_centred(None, 0) < 0 and lib.wann_dense_centred(None) == 0
    assert lib.wann_abi_version() == 5


def _regs(line):
    return int(line.split("vgpr+agpr")[1].split()[0])


def test_score_kernels_register_budget(wa):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_gemm_scoresILi"], capture_output=True, text=True, timeout=300)
    if out.returncode != 0 or not out.stdout.strip():
        pytest.skip("ROCm llvm tools not present")
    lines = out.stdout.splitlines()
    centred = [l for l in lines if re.search(r"k_gemm_scoresILi\d+ELb1E", l)]
    assert len(centred) == 16 and sum("dt_f16" in l for l in centred) == 8, centred  # eight strides in the float32 and the float16 unit
    for l in centred:
        assert _regs(l) <= 256 and int(l.split("scratch")[1].split()[0]) == 0 and int(l.split(" spill")[1].split()[0]) == 0, l
    record = open(os.path.join(REPO, "profiles", "dense_centred_kernel_resources.txt")).read().split("## ")[1]
    parent = {l.split()[0]: _regs(l) for l in record.splitlines() if l.startswith("_Z")}
    now = {l.split()[0].replace("ELb0E", "E"): _regs(l) for l in lines if re.search(r"k_gemm_scoresILi\d+ELb0E", l)}
    assert len(parent) == 16 and now == parent, (parent, now)
