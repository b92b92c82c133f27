"""CPU: the per-index switch of the float8 long-row dense path (wann_set_dense_long_float8, `k_gemm_scores_f8slab`) without a
device: the C symbols on a null index, the row-class table with and without the switch, the kernel's register budget."""
import ctypes
import os
import subprocess
import sys

from util import REPO

F8, NONE, NARROW, LONG = 8, 0, 1, 3
LONG_ROWS, LONG_FLOAT8 = 1, 2  # the switches wann_test_dense_row_class assumes on


def test_a_null_index_and_the_row_classes(wa):
    """float8 with its switch: narrow to 128 elements, long to 2048, none beyond.  Without it float8 stops at 128, and the switch
    moves no other type: its answers with and without wann_set_dense_long_rows stay those tests/test_dense_long_bfloat16_api.py pins"""
    import rangefilteredann_amd
    lib = ctypes.CDLL(rangefilteredann_amd.lib_path())
    assert lib.wann_set_dense_long_float8(None, 1) < 0 and lib.wann_set_dense_long_float8(None, 0) < 0 and lib.wann_dense_long_float8(None) == 0
    cls = lib.wann_test_dense_row_class
    cls.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    for d in range(1, 2201):
        for dtype in (0, 1, 2, 3, 5, F8):
            before = [cls(dtype, d, 0), cls(dtype, d, LONG_ROWS)]
            want = [NARROW if d <= 128 else LONG if d <= 2048 else NONE] * 2 if dtype == F8 else before
            assert [cls(dtype, d, LONG_FLOAT8), cls(dtype, d, LONG_ROWS | LONG_FLOAT8)] == want, (dtype, d)
            assert dtype != F8 or before == [NARROW if d <= 128 else NONE] * 2, d


def test_library_holds_the_kernel_within_the_units_budget(wa):
    """once, at most 256 registers (the cap tests/test_float8.py holds the unit's kernels to), no scratch, no spilled register"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_gemm_scores_f8slab"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and len(out.stdout.splitlines()) == 1, out.stdout + out.stderr
    l = out.stdout
    assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256 and int(l.split("scratch")[1].split()[0]) == 0 and int(l.split(" spill")[1].split()[0]) == 0, l
