// f8_sanitize_test.cpp -- the host side of the float8 element type (WANN_DTYPE_F8, OCP E4M3) under address + undefined-behaviour
// sanitizers (a program of make sanitize): the conversions of wann_f8.h over every bit pattern both ways, the rounding rule's
// edges, the layout predicates of wann_row_types.h / wann_device.h / wann_gemm_device.h for d = 1 .. 10 000, the packing of a float8 index's rows
// and the refusal of NaN patterns.  CPU only; no HIP.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/wann.h"
#include "wann_build.h"
#include "wann_device.h"
#include "wann_f8.h"
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

// the value of a finite pattern by its definition, in double arithmetic
static double value_of(uint8_t b) {
  const int e = (b >> 3) & 15, m = b & 7;
  const double mag = e == 0 ? ldexp((double)m, -9) : ldexp(1.0 + m / 8.0, e - 7);
  return (b & 0x80) ? -mag : mag;
}

static void check_every_pattern() {
  int nans = 0;
  double largest = 0;
  for (uint32_t b = 0; b < 256; b++) {
    const float f = f8_to_float((uint8_t)b);
    if (f8_is_nan((uint8_t)b)) {
      nans++;
      CHECK(isnan(f) && signbit(f) == ((b & 0x80) != 0));
      CHECK(float_to_f8(f) == b);  // NaN stays the NaN pattern of its sign
      continue;
    }
    CHECK((double)f == value_of((uint8_t)b) && signbit(f) == ((b & 0x80) != 0));
    CHECK(float_to_f8(f) == b);  // every finite value is its own rounding, -0.0 and the subnormals included
    // a normal float32 with at most four significant bits: exact as a bfloat16 too, and no denormal mode touches it
    CHECK((b & 0x7f) == 0 || ((bits_of(f) >> 23) & 0xff) != 0);
    CHECK((bits_of(f) & 0xfffffu) == 0);
    if (fabs((double)f) > largest) largest = fabs((double)f);
  }
  CHECK(nans == 2 && largest == 448.0);
  CHECK(f8_to_float(0x01) == ldexpf(1.f, -9) && f8_to_float(0x07) == ldexpf(7.f, -9) && f8_to_float(0x08) == ldexpf(1.f, -6));
  CHECK(bits_of(f8_to_float(0x80)) == 0x80000000u && bits_of(f8_to_float(0x00)) == 0);
}

// nearest, ties to even, by search over the finite patterns (the definition, not the formula)
static uint8_t round_by_search(float f) {
  const uint8_t sign = signbit(f) ? 0x80 : 0;
  if (isnan(f) || isinf(f)) return sign | 0x7f;
  const double a = fabs((double)f);
  int best = 0;
  for (int b = 0; b < 0x7f; b++) {
    const double db = fabs(a - value_of((uint8_t)b)), dbest = fabs(a - value_of((uint8_t)best));
    if (db < dbest || (db == dbest && !(b & 1) && (best & 1))) best = b;
  }
  // beyond 448: the next step of the format would be 480 (an odd mantissa) -- only what is nearer to that leaves the range; the
  // tie, 464, goes to the even 448
  if (a > 448.0 && a - 448.0 > 480.0 - a) return sign | 0x7f;
  return sign | (uint8_t)best;
}

static void check_rounding() {
  struct { float in; uint8_t out; } cases[] = {
      {448.f, 0x7e}, {464.f, 0x7e}, {465.f, 0x7f}, {480.f, 0x7f}, {1e30f, 0x7f}, {-464.f, 0xfe}, {-465.f, 0xff},
      {ldexpf(1.f, -10), 0x00}, {ldexpf(1.01f, -10), 0x01}, {ldexpf(3.f, -10), 0x02}, {ldexpf(1.f, -9), 0x01}, {-ldexpf(1.f, -9), 0x81},
      {ldexpf(0.99f, -10), 0x00}, {-ldexpf(1.f, -10), 0x80}, {0.f, 0x00}, {-0.f, 0x80}, {INFINITY, 0x7f}, {-INFINITY, 0xff},
      {from_bits(1), 0x00}, {from_bits(0x807fffffu), 0x80}, {ldexpf(15.5f, -10), 0x08}, {ldexpf(15.f, -10), 0x08}, {ldexpf(13.f, -10), 0x06},
      {1.0625f, 0x38}, {1.1875f, 0x3a}, {1.0626f, 0x39}, {17.f, 0x58}, {19.f, 0x5a}};
  for (auto &c : cases) CHECK(float_to_f8(c.in) == c.out);
  CHECK(float_to_f8(NAN) == 0x7f || float_to_f8(NAN) == 0xff);
  // ties at every binade boundary and halfway between every pair of neighbours, and their float32 neighbours
  for (int b = 0; b < 0x7e; b++) {
    const float lo = f8_to_float((uint8_t)b), hi = f8_to_float((uint8_t)(b + 1)), mid = 0.5f * (lo + hi);  // (exact: five significant bits)
    for (float x : {mid, nextafterf(mid, 0.f), nextafterf(mid, 1e9f), nextafterf(lo, 1e9f), nextafterf(hi, 0.f)})
      for (float s : {1.f, -1.f}) CHECK(float_to_f8(s * x) == round_by_search(s * x));
    CHECK(float_to_f8(mid) == ((b & 1) ? b + 1 : b));
  }
  // a sweep over float32 bit patterns, both signs, float32 subnormals and the overflow range included
  for (uint64_t u = 0; u < (1ull << 32); u += 4099) {
    const float f = from_bits((uint32_t)u);
    if (isnan(f)) {
      CHECK(f8_is_nan(float_to_f8(f)) && (float_to_f8(f) & 0x80) == ((u >> 24) & 0x80));
      continue;
    }
    CHECK(float_to_f8(f) == round_by_search(f));
  }
}

static IndexView view_of(int dtype, int d, int kind = 1) {
  IndexView v{};
  v.dtype = dtype;
  v.d = d;
  v.kind = kind;
  v.stride = (int32_t)(dtype == WANN_DTYPE_F8 ? u8_widened_stride_words(d) : dtype == kRowsU8Widened ? u8_widened_stride_words(d) : two_byte_stride_words(d));
  return v;
}

static void check_layout() {
  static_assert(WANN_DTYPE_F8 == 8 && kRowsF8 == 8, "the element type is its own view type");
  static_assert(widened_rows(kRowsF8) && one_byte_widened_rows(kRowsF8) && !two_byte_rows(kRowsF8) && upcast_built(kRowsF8), "float8 rows");
  static_assert(one_byte_widened_rows(kRowsU8Widened) && !upcast_built(kRowsU8Widened) && !one_byte_widened_rows(4) && !widened_rows(4) &&
                    !one_byte_widened_rows(WANN_DTYPE_U8),
                "nothing else changed; 4 is unassigned");
  static_assert(u8_widened_stride_words(1) == 16 && u8_widened_stride_words(64) == 16 && u8_widened_stride_words(65) == 32, "64-byte rows");
  for (int d = 1; d <= 10000; d++) {
    const IndexView f = view_of(WANN_DTYPE_F8, d), b = view_of(WANN_DTYPE_BF16, d), w = view_of(kRowsU8Widened, d);
    CHECK(f.stride * 4 == (d + 63) / 64 * 64 && f.stride == w.stride);  // d bytes padded to a multiple of 64
    CHECK(query_words(f) == ((d + 15) & ~15) && query_words(f) == query_words(b));
    CHECK(brute_lds_bytes(query_words(f), 10) == brute_lds_bytes(query_words(b), 10));
    CHECK(dense_row_class(f) == (d <= 128 ? kRowsNarrow : kRowsNone));
    // the scan: staged where the rows are sorted and a row fits, the plain kernel for the PrefilterIndex -- never more LDS than a CU has
    // unless the plain scan of the other widened types exceeds it too
    const IndexView p = view_of(WANN_DTYPE_F8, d, 0);
    CHECK(!scan_staged(p, 10) && scan_lds_bytes(p, 10) == brute_lds_bytes(query_words(b), 10));
    CHECK(scan_lds_bytes(f, 10) >= brute_lds_bytes(query_words(f), 10));
    CHECK((scan_lds_bytes(f, 10) <= kLdsPerWorkgroup) == (brute_lds_bytes(query_words(b), 10) <= kLdsPerWorkgroup));
    CHECK((scan_lds_bytes(f, 1024) <= kLdsPerWorkgroup) == (brute_lds_bytes(query_words(b), 1024) <= kLdsPerWorkgroup));
    CHECK(scan_staged(w, 10));  // (the one-byte shadow rows keep their one kernel)
  }
}

static void check_packing_and_refusal() {
  for (int d : {1, 4, 31, 32, 33, 64, 65, 100, 200}) {
    const int64_t n = 7, stride = ((d * 4 + 63) / 64) * 16, words = u8_widened_stride_words(d);
    std::vector<uint8_t> pat((size_t)n * d);
    for (size_t i = 0; i < pat.size(); i++) {
      pat[i] = (uint8_t)(i * 37 + 11);
      if (f8_is_nan(pat[i])) pat[i] = 0x80;
    }
    CHECK(f8_first_nan_row(pat.data(), n, d) == -1);
    std::vector<float> up((size_t)n * stride, 0.f), rows((size_t)n * words, 0.f);
    for (int64_t r = 0; r < n; r++)
      for (int j = 0; j < d; j++) up[(size_t)(r * stride + j)] = f8_to_float(pat[(size_t)(r * d + j)]);
    pack_f8_rows(up.data(), n, d, stride, words, 2, rows.data());
    std::vector<float> natural = rows;
    interleave_u8_rows(rows.data(), n, words, 2);
    const uint8_t *nat = reinterpret_cast<const uint8_t *>(natural.data()), *dev = reinterpret_cast<const uint8_t *>(rows.data());
    for (int64_t r = 0; r < n; r++)
      for (int64_t e = 0; e < words * 4; e++) {
        CHECK(nat[r * words * 4 + e] == (e < d ? pat[(size_t)(r * d + e)] : 0));
        CHECK(dev[r * words * 4 + u8_row_position(e)] == nat[r * words * 4 + e]);
      }
    // a NaN pattern anywhere names its row; 0x7f and 0xff alike
    for (uint8_t bad : {(uint8_t)0x7f, (uint8_t)0xff})
      for (int64_t at : {(int64_t)0, (int64_t)(3 * d + d / 2), (int64_t)(n * d - 1)}) {
        std::vector<uint8_t> q = pat;
        q[(size_t)at] = bad;
        CHECK(f8_first_nan_row(q.data(), n, d) == at / d);
      }
  }
}

int main() {
  check_every_pattern();
  check_rounding();
  check_layout();
  check_packing_and_refusal();
  if (failures) {
    fprintf(stderr, "f8_sanitize_test: %d check(s) failed\n", failures);
    return 1;
  }
  printf("F8_SANITIZE_OK\n");
  return 0;
}
