// bf16_sanitize_test.cpp -- the host side of the bfloat16 element type (WANN_DTYPE_BF16) under address + undefined-behaviour
// sanitizers (make sanitize, third program): the conversions of wann_bf16.h over every bit pattern, the rounding rule's edges,
// and the layout predicate of wann_row_types.h, which must treat bfloat16 rows exactly as float16 rows.  CPU only; no HIP.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/wann.h"
#include "wann_bf16.h"
#include "wann_device.h"
#include "wann_gemm_device.h"

using namespace wann;

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      failures++;                                                      \
    }                                                                  \
  } while (0)

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static void check_every_pattern() {
  int nans = 0;
  for (uint32_t b = 0; b < 65536; b++) {
    const float f = bf16_to_float((uint16_t)b);
    CHECK(bits_of(f) == b << 16);  // the widening is a shift
    const bool nan = (b & 0x7f80u) == 0x7f80u && (b & 0x7fu) != 0;
    const uint16_t back = float_to_bf16(f);
    if (nan) {
      nans++;
      CHECK(isnan(f) && isnan(bf16_to_float(back)));
      CHECK((back & 0x7fc0u) == 0x7fc0u && (back & 0x8000u) == (b & 0x8000u));  // quiet, sign kept
    } else {
      CHECK(back == b);
      CHECK(bits_of(two_byte_to_float(WANN_DTYPE_BF16, (uint16_t)b)) == b << 16);
      CHECK(float_to_two_byte(WANN_DTYPE_BF16, f) == b);
    }
  }
  CHECK(nans == 2 * 127);
  // the float16 conversions are still reached by their own code
  CHECK(two_byte_to_float(WANN_DTYPE_F16, 0x3c00) == 1.0f && float_to_two_byte(WANN_DTYPE_F16, 1.0f) == 0x3c00);
  CHECK(two_byte_to_float(WANN_DTYPE_BF16, 0x3f80) == 1.0f && float_to_two_byte(WANN_DTYPE_BF16, 1.0f) == 0x3f80);
}

static void check_rounding_edges() {
  struct { uint32_t in; uint16_t out; } cases[] = {
      {0x3f808000u, 0x3f80}, {0x3f818000u, 0x3f82},  // exact ties: to the even neighbour, down and up
      {0xbf808000u, 0xbf80}, {0xbf818000u, 0xbf82},
      {0x3f808001u, 0x3f81}, {0x3f807fffu, 0x3f80},
      {0x7f7f7fffu, 0x7f7f}, {0x7f7f8000u, 0x7f80},  // the last magnitude that stays finite, the first that becomes infinity
      {0xff7f7fffu, 0xff7f}, {0xff7f8000u, 0xff80}, {0x7f7fffffu, 0x7f80},
      {0x7f800000u, 0x7f80}, {0xff800000u, 0xff80},  // infinities stay
      {0x00000000u, 0x0000}, {0x80000000u, 0x8000},
      {0x00000001u, 0x0000}, {0x00008000u, 0x0000}, {0x00008001u, 0x0001}, {0x00018000u, 0x0002},  // float32 subnormals
      {0x007fffffu, 0x0080}, {0x80400000u, 0x8040},
      {0x7fc00000u, 0x7fc0}, {0xffc00000u, 0xffc0}, {0x7f800001u, 0x7fc0}, {0xff800001u, 0xffc0}, {0xffffffffu, 0xffc0}};  // NaN
  for (auto &c : cases) CHECK(float_to_bf16(from_bits(c.in)) == c.out);
  // the formula on a sweep of bit patterns, carries into the exponent included
  for (uint64_t u = 0; u < (1ull << 32); u += 7919) {
    const uint32_t a = (uint32_t)u & 0x7fffffffu;
    if (a > 0x7f800000u) continue;
    const uint16_t want = (uint16_t)(((uint64_t)(uint32_t)u + 0x7fffu + (((uint32_t)u >> 16) & 1u)) >> 16);
    CHECK(float_to_bf16(from_bits((uint32_t)u)) == want);
  }
}

static IndexView view_of(int dtype, int d) {
  IndexView v{};
  v.dtype = dtype;
  v.d = d;
  v.stride = (int32_t)two_byte_stride_words(d);
  return v;
}

static void check_layout() {
  static_assert(two_byte_rows(WANN_DTYPE_F16) && two_byte_rows(WANN_DTYPE_BF16), "float16 and bfloat16 share the row layout");
  static_assert(!two_byte_rows(WANN_DTYPE_F32) && !two_byte_rows(WANN_DTYPE_U8) && !two_byte_rows(WANN_DTYPE_I8) && !two_byte_rows(4) &&
                    !two_byte_rows(6),
                "nothing else does; 4 is unassigned");
  static_assert(two_byte_stride_words(1) == 16 && two_byte_stride_words(32) == 16 && two_byte_stride_words(33) == 32 &&
                    two_byte_stride_words(100) == 64 && two_byte_stride_words(128) == 64,
                "rows padded to 32 elements, counted in 32-bit words");
  // the shapes host_sanitize_test.cpp lists for the scan's LDS need, and every row length around its edges
  struct { int d, k; } shapes[] = {{128, 10}, {1024, 1024}, {3072, 10}, {4096, 1024}, {8192, 1024}, {8192, 65}, {2049, 10},
                                   {9952, 10}, {9953, 10}, {7936, 1024}, {7937, 1024}, {1, 1}, {16, 10}, {17, 10}, {100, 10}};
  for (auto &s : shapes) {
    const IndexView h = view_of(WANN_DTYPE_F16, s.d), b = view_of(WANN_DTYPE_BF16, s.d);
    CHECK(query_words(b) == query_words(h) && query_words(b) == ((s.d + 15) & ~15));
    CHECK(brute_lds_bytes(query_words(b), s.k) == brute_lds_bytes(query_words(h), s.k));
  }
  CHECK(brute_lds_bytes(query_words(view_of(WANN_DTYPE_BF16, 4096)), 1024) == 102400);  // (host_sanitize_test.cpp's float16 figure)
  for (int d = 1; d <= 10000; d++) {
    const IndexView h = view_of(WANN_DTYPE_F16, d), b = view_of(WANN_DTYPE_BF16, d);
    CHECK(b.stride == h.stride && query_words(b) == query_words(h));
    CHECK(brute_lds_bytes(query_words(b), 10) == brute_lds_bytes(query_words(h), 10));
    // the dense path: narrow rows of up to 128 elements, nothing beyond (float16 has its long class there)
    const DenseRows want = d <= 128 ? kRowsNarrow : kRowsNone;
    CHECK(dense_row_class(b) == want);
    if (d <= 128) CHECK(dense_row_class(h) == kRowsNarrow);
  }
}

int main() {
  check_every_pattern();
  check_rounding_edges();
  check_layout();
  if (failures) {
    fprintf(stderr, "bf16_sanitize_test: %d check(s) failed\n", failures);
    return 1;
  }
  printf("BF16_SANITIZE_OK\n");
  return 0;
}
