"""CPU: the per-index switch of the bfloat16 long-row dense path (wann_set_dense_long_rows, `k_gemm_scores_bfslab`) without a
device: the C symbols on a null index, the row-class table with and without the switch, the kernel's register budget.  (Return
values and defaults on real indexes of every kind and type: tests/test_gpu_dense_long_bfloat16.py.)"""
import ctypes
import os
import subprocess
import sys

from util import REPO

F32, U8, I8, F16, BF16, F8 = 0, 1, 2, 3, 5, 8
NONE, NARROW, WIDE, LONG = 0, 1, 2, 3


def test_a_null_index_and_the_row_classes(wa):
    """bfloat16 with the switch: narrow to 128 elements, long to 2048, none beyond; without it, and for every other type with or
    without it, the table is what it was (literal boundaries on the row of the float32 upcast / the padded bytes)"""
    import rangefilteredann_amd
    lib = ctypes.CDLL(rangefilteredann_amd.lib_path())
    assert lib.wann_set_dense_long_rows(None, 1) < 0 and lib.wann_set_dense_long_rows(None, 0) < 0 and lib.wann_dense_long_rows(None) == 0
    lib.wann_test_dense_row_class.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]

    def before(dtype, d):
        up, padded = (d + 15) & ~15, (d + 63) & ~63
        if dtype in (U8, I8):
            return NARROW if padded <= 512 else LONG if padded <= 2048 else NONE
        top = {F32: LONG, F16: LONG, BF16: NONE, F8: NONE}[dtype]
        return NARROW if up <= 128 else WIDE if dtype == F32 and up <= 512 else top if up <= 2048 else NONE
    for d in range(1, 2201):
        for dtype in (F32, U8, I8, F16, BF16, F8):
            assert lib.wann_test_dense_row_class(dtype, d, 0) == before(dtype, d), (dtype, d)
            want = before(dtype, d) if dtype != BF16 else NARROW if d <= 128 else LONG if d <= 2048 else NONE
            assert lib.wann_test_dense_row_class(dtype, d, 1) == want, (dtype, d)


def test_library_holds_the_kernel_within_the_units_budget(wa):
    """once, at most 256 registers (the cap tests/test_bfloat16.py holds the unit's kernels to), no scratch, no spilled register"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "k_gemm_scores_bfslab"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and len(out.stdout.splitlines()) == 1, out.stdout + out.stderr
    l = out.stdout
    assert int(l.split("vgpr+agpr")[1].split()[0]) <= 256 and int(l.split("scratch")[1].split()[0]) == 0 and int(l.split(" spill")[1].split()[0]) == 0, l
