"""CPU: the centred score kernels of wide float32 rows (`k_gemm_scores_wide_centred<2|3|4>`) as the library holds them: exactly
three instances, each within the 512 registers of one wave per SIMD, without scratch and without spills."""
import os
import subprocess
import sys

import pytest

from util import REPO


def test_three_instances_within_the_register_file(wa):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_gemm_scores_wide_centred"], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        pytest.skip("ROCm llvm tools not present")
    lines = out.stdout.splitlines()
    assert sorted(l.split()[0] for l in lines) == [f"_ZN4wann26k_gemm_scores_wide_centredILi{s}EEEvNS_8GemmArgsE" for s in (2, 3, 4)], lines
    for l in lines:
        assert int(l.split("vgpr+agpr")[1].split()[0]) <= 512 and int(l.split("scratch")[1].split()[0]) == 0 and int(l.split(" spill")[1].split()[0]) == 0, l
