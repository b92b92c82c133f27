// wann_kernels_h16.hip -- the search / scan kernels for the half shadow rows of a float32 index whose values are all binary16
// values: the float16 unit's kernels (every half converted exactly, scored in the float32 path's arithmetic and order) on rows
// whose halves are PAIRED inside every aligned group of 16 elements (wann_row_types.h h16_row_position), so that a lane fetches two
// of its blocks with one 16-byte load: see wann_kernels_body.inc and wann_wave.h (ld_pair).  An internal view type, not an
// element type of the C ABI (wann_row_types.h kRowsF16Paired): launch_search / search_occupancy are dispatched here, and
// launch_brute for the exact scans under wann_set_scan_rows (the plain k_brute).
#define WANN_DT 7
#include "wann_kernels_body.inc"
