// wann_kernels_bf16.hip -- the search / scan kernels of the window-filtered ANN engine for bfloat16 rows (half the vector
// bytes, float32's exponent range; every element widened by a shift and scored in the float32 path's arithmetic): one
// translation unit per element type of the point set, see wann_kernels_body.inc and wann_wave.h (rowblk_t).
#define WANN_DT 5
#include "wann_kernels_body.inc"
