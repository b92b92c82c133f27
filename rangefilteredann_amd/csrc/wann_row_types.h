// wann_row_types.h -- what a ROW TYPE is, stated once.  Plain C++ (no HIP): host code, the device passes and the stand-alone
// sanitizer programs include it, and every predicate, pitch, unit namespace and launcher lookup of the engine is derived from
// the one list below.  Adding a type: one entry here, a .hip stub per kind of unit it has, and the `#if` arms of the kernels
// that really differ.
//
// A row type is the value of IndexView::dtype: how the rows behind IndexView::points are stored and which unit's kernels read
// them.  Six are element types of the C ABI (wann.h WANN_DTYPE_*); 6 and 7 are INTERNAL view types, the shadow copies of a
// float32 index's rows, which no entry point accepts; 4 is unassigned and refused everywhere.
//
//   id            IndexView::dtype
//   unit          the namespace of the type's translation units (wann_kernels_*.hip, wann_gemm_kernels_*.hip, wann_build_kernels_*.hip)
//   abi           1: an element type the C ABI accepts (known_dtype)
//   caller bytes  of one element in the caller's arrays and host queries (element_bytes; 0: no caller ever holds such rows)
//   pitch         the device row pitch in 32-bit words (row_stride_words): Spec = the build spec's float32 stride, TwoByte =
//                 two_byte_stride_words(d), OneByte = u8_widened_stride_words(d) -- every row is zero padded to 64 bytes
//   layout        the order of the elements inside a device row: Natural, U8 (u8_row_position), H16 (h16_row_position)
//   byte-dot      uint8 / int8 rows, scored with v_dot4 by kernels built for more waves per SIMD (byte_rows, WANN_BYTE_ROWS)
//   two-byte      two-byte float rows (two_byte_rows, WANN_HALF_ROWS)
//   quad          one-byte rows in the interleaved layout, fetched 16 bytes at a time (one_byte_widened_rows, WANN_QUAD_ROWS)
//   upcast-built  the host rows (HostIndex::pts) are the exact float32 upcast of the caller's: both builders build from those
//   search / dense / build   the type has a unit of that kind (SearchUnit, GemmUnit, BuildUnit); a type without one is an
//                 error at the entry point, never another type's kernels
//
// "Widened" = two-byte or quad: rows narrower than float32 that are scored as their exact float32 upcast against an fp32 query.
#ifndef WANN_ROW_TYPES_H
#define WANN_ROW_TYPES_H
#include <stdint.h>

//                               X(id, unit,   abi, caller bytes, pitch, layout, byte-dot, two-byte, quad, upcast-built, search, dense, build)
#define WANN_ROW_TYPE_0(X, ...) X(0, dt_f32,  1, 4, Spec,    Natural, 0, 0, 0, 0, 1, 1, 1, __VA_ARGS__)
#define WANN_ROW_TYPE_1(X, ...) X(1, dt_u8,   1, 1, Spec,    Natural, 1, 0, 0, 0, 1, 1, 1, __VA_ARGS__)
#define WANN_ROW_TYPE_2(X, ...) X(2, dt_i8,   1, 1, Spec,    Natural, 1, 0, 0, 0, 1, 1, 1, __VA_ARGS__)
#define WANN_ROW_TYPE_3(X, ...) X(3, dt_f16,  1, 2, TwoByte, Natural, 0, 1, 0, 1, 1, 1, 0, __VA_ARGS__)
#define WANN_ROW_TYPE_5(X, ...) X(5, dt_bf16, 1, 2, TwoByte, Natural, 0, 1, 0, 1, 1, 1, 0, __VA_ARGS__)
#define WANN_ROW_TYPE_6(X, ...) X(6, dt_w8,   0, 0, OneByte, U8,      0, 0, 1, 0, 1, 1, 0, __VA_ARGS__)  // (dense: a score kernel only)
#define WANN_ROW_TYPE_7(X, ...) X(7, dt_h16,  0, 0, TwoByte, H16,     0, 1, 0, 0, 1, 0, 0, __VA_ARGS__)
#define WANN_ROW_TYPE_8(X, ...) X(8, dt_f8,   1, 1, OneByte, U8,      0, 0, 1, 1, 1, 1, 0, __VA_ARGS__)
// THE LIST: X is applied to every entry; what follows X is handed to it behind the entry's own fields
#define WANN_ROW_TYPES(...)                                                                                          \
  WANN_ROW_TYPE_0(__VA_ARGS__) WANN_ROW_TYPE_1(__VA_ARGS__) WANN_ROW_TYPE_2(__VA_ARGS__) WANN_ROW_TYPE_3(__VA_ARGS__) \
  WANN_ROW_TYPE_5(__VA_ARGS__) WANN_ROW_TYPE_6(__VA_ARGS__) WANN_ROW_TYPE_7(__VA_ARGS__) WANN_ROW_TYPE_8(__VA_ARGS__)

#define WANN_CAT_(a, b) a##b
#define WANN_CAT(a, b) WANN_CAT_(a, b)
// WANN_IF(flag)(text): the text where the flag (an entry's 0 / 1 field) is 1, nothing where it is 0
#define WANN_IF_0(...)
#define WANN_IF_1(...) __VA_ARGS__
#define WANN_IF(flag) WANN_CAT(WANN_IF_, flag)

namespace wann {

enum RowPitch { kPitchSpec, kPitchTwoByte, kPitchOneByte };
enum RowLayout { kLayoutNatural, kLayoutU8, kLayoutH16 };
struct RowType {
  int id;
  bool abi;
  int caller_bytes;
  RowPitch pitch;
  RowLayout layout;
  bool byte_dot, two_byte, quad, upcast_built, search, dense, build;
};
#define WANN_X_ROW(id, ns, abi, cb, pitch, layout, bd, tb, q, up, s, d, b, ...) \
  {id, abi != 0, cb, kPitch##pitch, kLayout##layout, bd != 0, tb != 0, q != 0, up != 0, s != 0, d != 0, b != 0},
constexpr RowType kRowTypes[] = {WANN_ROW_TYPES(WANN_X_ROW)};
#undef WANN_X_ROW
// an id the list does not hold (4, anything below 0 or beyond 8): no class, no caller bytes, no unit of any kind
constexpr RowType kNoRowType = {-1, false, 0, kPitchSpec, kLayoutNatural, false, false, false, false, false, false, false};
constexpr const RowType &row_type(int dtype) {
  for (const RowType &t : kRowTypes)
    if (t.id == dtype) return t;
  return kNoRowType;
}

// the ids, for code that has to name one: the C ABI's element types (wann.h WANN_DTYPE_* are these values) ...
constexpr int kRowsF32 = 0, kRowsU8 = 1, kRowsI8 = 2, kRowsF16 = 3, kRowsBF16 = 5;
// ... the two internal view types, and float8 (an element type of the C ABI that is its own view type)
// One-byte shadow rows of a float32 index (INTERNAL, never a WANN_DTYPE_* the C ABI accepts): every value is an integer 0 .. 255
// stored as a uint8 -- d bytes, zero padded to a multiple of 64 -- and the beam-search kernels of wann_kernels_w8.hip widen each
// byte exactly to the float32 it stands for.  k_search is launched on such a view, and k_brute under wann_set_scan_rows; under
// wann_set_dense_rows the dense path's k_gemm_scores too (wann_gemm_kernels_w8.hip: each byte widened to the bfloat16 it also is).
constexpr int kRowsU8Widened = 6;
// Half shadow rows of a float32 index (INTERNAL like 6): the float16 rows' values, pitch and padding with the halves of every
// aligned group of 16 elements PAIRED (h16_row_position); the kernels of wann_kernels_h16.hip read them, and every predicate
// treats such a view as a float16 one.
constexpr int kRowsF16Paired = 7;
// Float8 rows (wann.h WANN_DTYPE_F8, OCP E4M3 bit patterns): device rows with the one-byte shadow rows' pitch and LAYOUT; the
// kernels of wann_kernels_f8.hip / wann_gemm_kernels_f8.hip widen each byte exactly to the float32 (bfloat16) it stands for.
// Host arrays and cache inputs keep the natural order: interleave_u8_rows runs before the upload.
constexpr int kRowsF8 = 8;

constexpr bool known_dtype(int dtype) { return row_type(dtype).abi; }                   // the element types the C ABI accepts
constexpr int64_t element_bytes(int dtype) { return row_type(dtype).caller_bytes; }      // per element of the caller's points / host queries
constexpr bool byte_rows(int dtype) { return row_type(dtype).byte_dot; }
// two-byte float rows: float16 and bfloat16 share the row pitch and layout rules -- d elements in natural order, zero padded to
// a multiple of 32 (64 B) -- and the staged query's length; the half shadow rows share all of it but the order inside a group of 16
constexpr bool two_byte_rows(int dtype) { return row_type(dtype).two_byte; }
constexpr bool one_byte_widened_rows(int dtype) { return row_type(dtype).quad; }
constexpr bool widened_rows(int dtype) { return two_byte_rows(dtype) || one_byte_widened_rows(dtype); }
constexpr bool upcast_built(int dtype) { return row_type(dtype).upcast_built; }

// The build spec's stride: the pitch of the HOST rows (HostIndex::pts) in 32-bit words -- d stored elements, the caller's or
// their float32 upcast, zero padded to 64 bytes (point_range.h:39-44).  The device pitch of float32 and byte-dot rows.
constexpr int64_t spec_stride_words(int dtype, int64_t d) { return ((d * (upcast_built(dtype) ? 4 : element_bytes(dtype)) + 63) / 64) * 16; }
// the pitch rules of the other rows, in 32-bit words
constexpr int64_t two_byte_stride_words(int64_t d) { return ((d * 2 + 63) / 64) * 16; }
constexpr int64_t u8_widened_stride_words(int64_t d) { return ((d + 63) / 64) * 16; }
// the device row pitch of a type's rows of d elements; f32_stride: the build spec's stride (float32 and byte-dot rows keep it)
constexpr int64_t row_stride_words(int dtype, int64_t d, int64_t f32_stride) {
  return row_type(dtype).pitch == kPitchTwoByte ? two_byte_stride_words(d) : row_type(dtype).pitch == kPitchOneByte ? u8_widened_stride_words(d) : f32_stride;
}
// 32-bit words of a staged query (fp32, zero padded; the LDS the kernels reserve for it): the stride for float32 / byte-dot
// rows, the float32 row length (d rounded up to 16) for widened rows -- the same LDS layout as the float32 index
constexpr int query_words(int dtype, int d, int stride) { return widened_rows(dtype) ? ((d + 15) & ~15) : stride; }

// THE LAYOUT U8 (the one-byte shadow rows' device copy, wann_index::d_bytes / byte_view, and float8 rows), stated once: a row
// keeps its pitch, and inside every aligned group of 32 elements the bytes are permuted -- element e of a row sits at byte
// u8_row_position(e) of it.  A row BLOCK is four consecutive elements (wann_wave.h); lane h of a lane pair owns the blocks
// 8 b + 4 h, and for b = 4 c .. 4 c + 3 those four blocks are the 16 contiguous bytes at 32 c + 16 h: one 16-byte load per lane
// brings four blocks (a QUAD), a lane pair covers 32 contiguous bytes per load instruction.  The padded row is a whole number of
// quads and its padding is zero, so a whole quad may always be loaded.  pack_u8_rows (wann_build.h) writes the natural order,
// interleave_u8_rows turns it into this one before the upload; wann_byte_row_position (wann.h) is this function.
constexpr int64_t u8_row_position(int64_t e) { return 32 * (e >> 5) + 16 * ((e >> 2) & 1) + 4 * ((e >> 3) & 3) + (e & 3); }
// THE LAYOUT H16 (the half shadow rows' device copy, wann_index::d_half / search_view), stated once: a row keeps its pitch, and
// inside every aligned group of 16 elements the halves are permuted -- element e of a row sits at half h16_row_position(e) of
// it.  Lane h of a lane pair owns the blocks 8 b + 4 h (wann_wave.h), and its two blocks b = 2 c and 2 c + 1 are the 16
// contiguous bytes at byte 32 c + 16 h of the row: one 16-byte load per lane brings two blocks (a PAIR).  Rows stay padded with
// zeros to 64 bytes, so every pair exists and is 16-byte aligned.  interleave_h16_rows (wann_build.h) turns natural-order rows
// into this order before the upload; wann_half_row_position (wann.h) is this function.  Native float16 / bfloat16 indexes keep
// the natural order: the dense path, the build kernels and finalisation read those rows.
constexpr int64_t h16_row_position(int64_t e) { return 16 * (e >> 4) + 8 * ((e >> 2) & 1) + 4 * ((e >> 3) & 1) + (e & 3); }

}  // namespace wann

// The launchers of a kind of unit (search / dense / build), one struct of function pointers per unit reached through an
// accessor in the unit's namespace.  WANN_UNIT_LOOKUP(kind, Unit, accessor, lookup) declares ns::accessor() for every type that
// has a unit of that kind and defines lookup(dtype): that unit, or null for a type without one (inside namespace wann).
#define WANN_UNIT_search(s, d, b) s
#define WANN_UNIT_dense(s, d, b) d
#define WANN_UNIT_build(s, d, b) b
#define WANN_X_UNIT_DECL(id, ns, abi, cb, pitch, layout, bd, tb, q, up, s, d, b, kind, Unit, accessor) \
  WANN_IF(WANN_UNIT_##kind(s, d, b))(namespace ns { const Unit &accessor(); })
#define WANN_X_UNIT_CASE(id, ns, abi, cb, pitch, layout, bd, tb, q, up, s, d, b, kind, Unit, accessor) \
  WANN_IF(WANN_UNIT_##kind(s, d, b))(case id: return &ns::accessor();)
#define WANN_UNIT_LOOKUP(kind, Unit, accessor, lookup)   \
  WANN_ROW_TYPES(WANN_X_UNIT_DECL, kind, Unit, accessor) \
  inline const Unit *lookup(int dtype) {                 \
    switch (dtype) {                                     \
      WANN_ROW_TYPES(WANN_X_UNIT_CASE, kind, Unit, accessor) \
      default: return nullptr;                           \
    }                                                    \
  }

#endif  // WANN_ROW_TYPES_H

// (outside the include guard: wann_wave.h includes this header again once it has given a unit without a WANN_DT the float32 one)
// A translation unit that defines WANN_DT (a kernel unit of one row type) gets the type's namespace, the template parameter
// its kernels carry and its class flags from the same list.  WANN_DT_TPARAM: the kernels of the widened types carry the type
// as a last template argument (k_search<METRIC, KIND, 3>), so their symbols differ from the float32 / byte-dot kernels' in more
// than the namespace, and per-type tools and tests that select the reference's three types by the kernel name's template
// arguments keep selecting exactly those; for types 0, 1 and 2 it is empty.
#if defined(WANN_DT) && !defined(WANN_DT_ENTRY)
#define WANN_X_NS(id, ns, ...) ns
#define WANN_X_BYTE(id, ns, abi, cb, pitch, layout, bd, tb, q, ...) bd
#define WANN_X_HALF(id, ns, abi, cb, pitch, layout, bd, tb, q, ...) tb
#define WANN_X_QUAD(id, ns, abi, cb, pitch, layout, bd, tb, q, ...) q
#define WANN_X_TPARAM(id, ns, abi, cb, pitch, layout, bd, tb, q, ...) WANN_CAT(WANN_CAT(WANN_TPARAM_, tb), q)
#define WANN_TPARAM_00
#define WANN_TPARAM_10 , int ROWS_DT = WANN_DT
#define WANN_TPARAM_01 , int ROWS_DT = WANN_DT
#define WANN_DT_ENTRY WANN_CAT(WANN_ROW_TYPE_, WANN_DT)
#define WANN_DT_NS WANN_DT_ENTRY(WANN_X_NS, )
#define WANN_DT_TPARAM WANN_DT_ENTRY(WANN_X_TPARAM, )
#define WANN_BYTE_ROWS WANN_DT_ENTRY(WANN_X_BYTE, )
#define WANN_HALF_ROWS WANN_DT_ENTRY(WANN_X_HALF, )
#define WANN_QUAD_ROWS WANN_DT_ENTRY(WANN_X_QUAD, )
#define WANN_WIDENED_ROWS (WANN_HALF_ROWS || WANN_QUAD_ROWS)
static_assert(WANN_BYTE_ROWS == wann::byte_rows(WANN_DT) && WANN_HALF_ROWS == wann::two_byte_rows(WANN_DT) &&
                  WANN_QUAD_ROWS == wann::one_byte_widened_rows(WANN_DT) && WANN_WIDENED_ROWS == wann::widened_rows(WANN_DT),
              "the class macros of this unit are the predicates of its row type");
static_assert(wann::row_type(WANN_DT).id == WANN_DT, "WANN_DT names an entry of the list");
#endif
