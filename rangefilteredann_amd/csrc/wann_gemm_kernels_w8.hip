// wann_gemm_kernels_w8.hip -- the dense prefilter path's score kernel for the one-byte shadow rows of a float32 index whose
// values are all integers 0 .. 255 (wann_set_dense_rows; an internal view type, wann_row_types.h kRowsU8Widened): see
// wann_gemm_kernels_body.inc; the score kernel is wann_gemm_kernels_w8.inc.  The unit holds no other kernel.
#define WANN_DT 6
#include "wann_gemm_kernels_body.inc"
