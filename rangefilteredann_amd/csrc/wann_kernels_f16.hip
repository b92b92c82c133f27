// wann_kernels_f16.hip -- the search / scan kernels of the window-filtered ANN engine for float16 rows (half the vector
// bytes; every element converted exactly and scored in the float32 path's arithmetic): one translation unit per element type
// of the point set, see wann_kernels_body.inc and wann_wave.h (rowblk_t).
#define WANN_DT 3
#include "wann_kernels_body.inc"
