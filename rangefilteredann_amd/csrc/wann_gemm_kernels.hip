// wann_gemm_kernels.hip -- the dense prefilter path (shared-window PrefilterIndex batches on the matrix cores) for float32 rows
// (+ the type-independent grouping kernels and the dispatchers): one translation unit per element type of the point set, see
// wann_gemm_kernels_body.inc.
#define WANN_DT 0
#include "wann_gemm_kernels_body.inc"
