// wann_kernels_f8.hip -- the search / scan kernels of the window-filtered ANN engine for float8 rows (OCP E4M3, wann.h
// WANN_DTYPE_F8: a quarter of the vector bytes; every byte widened exactly by v_cvt_pk_f32_fp8 and scored in the float32
// path's arithmetic against the fp32 query).  The rows have the one-byte shadow rows' interleaved layout, and the unit is that
// unit's blocks, quads, loaders and lane pairing with another cvt_blk: see wann_kernels_body.inc and wann_wave.h (rowblk_t).
// An element type of the C ABI, so a full unit: k_search of every kind, k_brute_staged for the sorted kinds' contiguous scans
// and the plain k_brute for the PrefilterIndex's gathered rows.
#define WANN_DT 8
#include "wann_kernels_body.inc"
