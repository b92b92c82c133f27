// wann_gemm_kernels_f16.hip -- the dense prefilter path for float16 rows: one translation unit per element type of the point
// set, see wann_gemm_kernels_body.inc.
#define WANN_DT 3
#include "wann_gemm_kernels_body.inc"
