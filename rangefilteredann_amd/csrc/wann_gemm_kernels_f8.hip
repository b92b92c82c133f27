// wann_gemm_kernels_f8.hip -- the dense prefilter path for float8 rows (OCP E4M3, wann.h WANN_DTYPE_F8): one translation unit
// per element type of the point set, see wann_gemm_kernels_body.inc.  The score kernel is wann_gemm_kernels_w8.inc's -- the
// bfloat16 kernel behind a byte fetch -- with each byte widened to the bfloat16 it also is; unlike the unit of the one-byte
// shadow rows this one is a full unit: norms, re-rank, cover re-rank and rescue read the float8 rows, there are no others.
#define WANN_DT 8
#include "wann_gemm_kernels_body.inc"
