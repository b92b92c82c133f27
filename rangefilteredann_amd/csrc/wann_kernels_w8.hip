// wann_kernels_w8.hip -- the beam-search kernels for the one-byte shadow rows of a float32 index whose values are all integers
// 0 .. 255 (a quarter of the vector bytes; every byte widened unsigned to the float32 it was made from and scored in the
// float32 path's arithmetic against the fp32 query): see wann_kernels_body.inc and wann_wave.h (rowblk_t).  An internal view
// type, not an element type of the C ABI: launch_search / search_occupancy are dispatched here, and launch_brute for the exact
// scans under wann_set_scan_rows (k_brute_staged, the unit's one scan kernel) (wann_row_types.h kRowsU8Widened).
#define WANN_DT 6
#include "wann_kernels_body.inc"
