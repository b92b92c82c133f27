// wann_gemm_kernels_u8.hip -- the dense prefilter path for uint8 rows: one translation unit per element type of the point
// set, see wann_gemm_kernels_body.inc.
#define WANN_DT 1
#include "wann_gemm_kernels_body.inc"
