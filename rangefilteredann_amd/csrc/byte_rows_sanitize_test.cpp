// byte_rows_sanitize_test.cpp -- the host side of the one-byte shadow rows of a float32 index (wann_set_byte_rows) under address
// + undefined-behaviour sanitizers (make sanitize, fourth program): the eligibility rule (rows_u8_exact), the packing of a
// point set into zero-padded byte rows, and the layout predicates of wann_row_types.h.  CPU only; no HIP.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/wann.h"
#include "wann_build.h"
#include "wann_device.h"

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

static bool one(float v) { return rows_u8_exact(&v, 1, 1, 1, 1); }

// every integer -300 .. 300 and the halves between them: exactly the integers 0 .. 255 qualify; then the special values
static void check_rule() {
  for (int i = -600; i <= 600; i++) {
    const float v = 0.5f * (float)i;
    const bool want = (i % 2 == 0) && i >= 0 && i <= 510;
    if (one(v) != want) {
      fprintf(stderr, "FAILED rule at %g\n", v);
      failures++;
    }
  }
  CHECK(one(0.0f));
  CHECK(!one(-0.0f));  // (on bits: (float)(uint8_t)-0.0 is +0.0)
  CHECK(from_bits(0x80000000u) == 0.0f && !one(from_bits(0x80000000u)));
  const uint32_t refused[] = {0x00000001u /* 2^-149 */, 0x80000001u, 0x00800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u,
                              0x7fc00000u, 0xffc00000u, 0x7fc02000u, 0x7f800001u, 0xff800001u, 0x437f0001u /* just above 255 */,
                              0x437effffu /* just below 255 */, 0x43800000u /* 256 */, 0x4f800000u /* 2^32 */, 0x7149f2cau /* 1e30 */};
  for (uint32_t b : refused) {
    if (one(from_bits(b))) {
      fprintf(stderr, "FAILED: bits %08x accepted\n", b);
      failures++;
    }
  }
  // one bad value at the start, in the middle and at the end of a padded array, with several threads; the stride is honoured
  const int64_t n = 1000, d = 20, stride = 32;
  std::vector<float> a((size_t)n * stride, 0.5f);  // (the padding holds values that would fail: it is never read)
  for (int64_t r = 0; r < n; r++)
    for (int64_t j = 0; j < d; j++) a[(size_t)(r * stride + j)] = (float)((r * 7 + j * 13) % 256);
  CHECK(rows_u8_exact(a.data(), n, d, stride, 4));
  const int64_t at[3] = {0, 500 * stride + 3, (n - 1) * stride + d - 1};
  for (int64_t p : at) {
    const float was = a[(size_t)p];
    a[(size_t)p] = 256.f;
    CHECK(!rows_u8_exact(a.data(), n, d, stride, 4));
    a[(size_t)p] = was;
  }
  CHECK(rows_u8_exact(a.data(), n, d, stride, 4));
  CHECK(rows_u8_exact(nullptr, 0, d, stride, 4));  // (the empty set)
}

// the packing: row r's values as bytes in natural order, every padding byte zero, the stride of the view
static void check_packing() {
  static_assert(u8_widened_stride_words(1) == 16 && u8_widened_stride_words(20) == 16 && u8_widened_stride_words(64) == 16 &&
                    u8_widened_stride_words(65) == 32 && u8_widened_stride_words(128) == 32 && u8_widened_stride_words(200) == 64,
                "64-byte padded rows, counted in 32-bit words");
  const int64_t dims[] = {1, 20, 64, 65, 128, 200};
  for (int64_t d : dims) {
    const int64_t n = 37, stride = (d + 15) / 16 * 16, words = u8_widened_stride_words(d);
    CHECK(words == 16 * ((d + 63) / 64) && words * 4 >= d && (words * 4) % 64 == 0);
    std::vector<float> pts((size_t)(n * stride), 0.f);
    for (int64_t r = 0; r < n; r++)
      for (int64_t j = 0; j < d; j++) pts[(size_t)(r * stride + j)] = (float)((r * 31 + j * 17 + 128) % 256);
    CHECK(rows_u8_exact(pts.data(), n, d, stride, 3));
    std::vector<float> rows((size_t)(n * words), 0.f);  // (exactly n rows: a write past the last row is the sanitizer's to find)
    pack_u8_rows(pts.data(), n, d, stride, words, 3, rows.data());
    const uint8_t *b = reinterpret_cast<const uint8_t *>(rows.data());
    bool values = true, padding = true, high = false;
    for (int64_t r = 0; r < n; r++)
      for (int64_t j = 0; j < words * 4; j++) {
        const uint8_t got = b[r * words * 4 + j];
        if (j < d) {
          values = values && (float)got == pts[(size_t)(r * stride + j)];
          high = high || got >= 128;
        } else {
          padding = padding && got == 0;
        }
      }
    CHECK(values);
    CHECK(padding);
    CHECK(high);  // (values of 128 and above occur: a signed narrowing would show)
  }
}

// the predicates: a byte view stages its query as the half view of the same index does -- the float32 upcast's length --
// and is no two-byte row; 6 is no element type of the C ABI
static void check_predicates() {
  static_assert(kRowsU8Widened == 6, "the internal view type");
  static_assert(widened_rows(WANN_DTYPE_F16) && widened_rows(WANN_DTYPE_BF16) && widened_rows(kRowsU8Widened), "rows scored as their upcast");
  static_assert(!widened_rows(WANN_DTYPE_F32) && !widened_rows(WANN_DTYPE_U8) && !widened_rows(WANN_DTYPE_I8) && !widened_rows(4), "the others");
  static_assert(!two_byte_rows(kRowsU8Widened), "one byte per element");
  static_assert(kRowsU8Widened != WANN_DTYPE_F32 && kRowsU8Widened != WANN_DTYPE_U8 && kRowsU8Widened != WANN_DTYPE_I8 &&
                    kRowsU8Widened != WANN_DTYPE_F16 && kRowsU8Widened != WANN_DTYPE_BF16,
                "not a public element type");
  const int64_t dims[] = {1, 20, 64, 65, 100, 128, 200};
  for (int64_t d : dims) {
    IndexView f{}, h{}, b{};
    f.d = h.d = b.d = (int32_t)d;
    f.dtype = WANN_DTYPE_F32;
    f.stride = (int32_t)((d + 15) / 16 * 16);
    h.dtype = WANN_DTYPE_F16;
    h.stride = (int32_t)two_byte_stride_words(d);
    b.dtype = kRowsU8Widened;
    b.stride = (int32_t)u8_widened_stride_words(d);
    CHECK(query_words(b) == query_words(h));
    CHECK(query_words(b) == query_words(f));  // (the float32 index's own LDS layout)
    CHECK(query_words(b) == (int)((d + 15) & ~(int64_t)15));
  }
}

int main() {
  check_rule();
  check_packing();
  check_predicates();
  if (failures) {
    fprintf(stderr, "byte_rows_sanitize_test: %d failures\n", failures);
    return 1;
  }
  printf("byte_rows_sanitize_test ok\n");
  return 0;
}
