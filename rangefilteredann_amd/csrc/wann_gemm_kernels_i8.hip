// wann_gemm_kernels_i8.hip -- the dense prefilter path for int8 rows: one translation unit per element type of the point
// set, see wann_gemm_kernels_body.inc.
#define WANN_DT 2
#include "wann_gemm_kernels_body.inc"
