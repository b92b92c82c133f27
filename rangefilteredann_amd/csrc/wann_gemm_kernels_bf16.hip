// wann_gemm_kernels_bf16.hip -- the dense prefilter path for bfloat16 rows: one translation unit per element type of the point
// set, see wann_gemm_kernels_body.inc; the score kernel is wann_gemm_kernels_bf16.inc.
#define WANN_DT 5
#include "wann_gemm_kernels_body.inc"
