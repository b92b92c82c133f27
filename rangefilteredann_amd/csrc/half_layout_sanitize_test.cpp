// half_layout_sanitize_test.cpp -- the layout of the device copy of the half shadow rows (h16_row_position in wann_row_types.h,
// interleave_h16_rows in wann_build.cpp) under address + undefined-behaviour sanitizers (make sanitize): the half rows of a
// point set, paired in buffers of exactly n rows, hold x[r][e] at half h16_row_position(e) of row r and zero in every other
// half, and the permutation's inverse gives the natural-order rows back.  CPU only; no HIP.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "../../include/wann.h"
#include "wann_build.h"
#include "wann_device.h"
#include "wann_half.h"

using namespace wann;

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      failures++;                                                      \
    }                                                                  \
  } while (0)

// the element stored at half `pos` of a row: the inverse of h16_row_position, written out on its own
static int64_t element_at(int64_t pos) {
  const int64_t r = pos & 15;
  return 16 * (pos >> 4) + 8 * ((r >> 2) & 1) + 4 * ((r >> 3) & 1) + (r & 3);
}

// the rule itself: a permutation of every aligned group of 16, pairs of lane h's blocks contiguous and in order
static void check_rule() {
  static_assert(h16_row_position(0) == 0 && h16_row_position(3) == 3 && h16_row_position(4) == 8 && h16_row_position(8) == 4 &&
                    h16_row_position(12) == 12 && h16_row_position(15) == 15 && h16_row_position(16) == 16 && h16_row_position(20) == 24,
                "the paired layout");
  static_assert(kRowsF16Paired == 7 && two_byte_rows(kRowsF16Paired) && widened_rows(kRowsF16Paired) && kRowsF16Paired != kRowsU8Widened,
                "the internal view type behaves as float16 rows");
  for (int64_t e = 0; e < 4096; e++) {
    const int64_t p = h16_row_position(e);
    CHECK(p == 16 * (e >> 4) + 8 * ((e >> 2) & 1) + 4 * ((e >> 3) & 1) + (e & 3));
    CHECK((p >> 4) == (e >> 4));
    CHECK(element_at(p) == e);
    CHECK(p == 16 * (e / 16) + h16_row_position(e % 16));
  }
  for (int64_t g = 0; g < 256; g++) {
    bool seen[16] = {};
    for (int64_t e = 16 * g; e < 16 * g + 16; e++) seen[h16_row_position(e) - 16 * g] = true;
    for (bool s : seen) CHECK(s);
  }
  for (int64_t c = 0; c < 256; c++)
    for (int64_t h = 0; h < 2; h++)
      for (int64_t i = 0; i < 2; i++)
        for (int64_t j = 0; j < 4; j++) CHECK(h16_row_position(16 * c + 8 * i + 4 * h + j) == 16 * c + 8 * h + 4 * i + j);
}

static void check_rows() {
  const int64_t dims[] = {1, 8, 16, 17, 20, 32, 33, 40, 100, 128, 136, 200, 256, 264};
  for (int64_t d : dims) {
    const int64_t n = 37, words = two_byte_stride_words(d), pitch = words * 2;  // (pitch in halves)
    CHECK(pitch % 32 == 0 && pitch >= d);
    std::vector<float> x((size_t)(n * d));
    for (int64_t r = 0; r < n; r++)
      for (int64_t e = 0; e < d; e++) x[(size_t)(r * d + e)] = (float)(1 + (r * 31 + e * 17) % 1500) / 8.f;  // (never 0: a value in a padding half shows)
    std::vector<float> nat((size_t)(n * words), 0.f);  // (exactly n rows: an access past the last row is the sanitizer's to find)
    for (int64_t r = 0; r < n; r++) {
      uint16_t *dst = reinterpret_cast<uint16_t *>(nat.data() + r * words);
      for (int64_t e = 0; e < d; e++) dst[e] = float_to_half(x[(size_t)(r * d + e)]);
    }
    std::vector<float> rows(nat);
    interleave_h16_rows(rows.data(), n, words, 3);
    const uint16_t *b = reinterpret_cast<const uint16_t *>(rows.data());
    const uint16_t *nb = reinterpret_cast<const uint16_t *>(nat.data());
    bool values = true, zeros = true, inverse = true;
    std::vector<uint8_t> owned((size_t)pitch);
    for (int64_t r = 0; r < n; r++) {
      std::fill(owned.begin(), owned.end(), (uint8_t)0);
      for (int64_t e = 0; e < d; e++) {
        const int64_t p = h16_row_position(e);
        if (p < 0 || p >= pitch) {
          values = false;
          continue;
        }
        owned[(size_t)p] = 1;
        values = values && half_to_float(b[r * pitch + p]) == x[(size_t)(r * d + e)];
      }
      for (int64_t p = 0; p < pitch; p++) {
        if (!owned[(size_t)p]) zeros = zeros && b[r * pitch + p] == 0;
        inverse = inverse && b[r * pitch + p] == nb[r * pitch + element_at(p)];
      }
    }
    CHECK(values);
    CHECK(zeros);
    CHECK(inverse);
    // ... and undone half by half, the natural-order rows again
    std::vector<uint16_t> back((size_t)(n * pitch));
    for (int64_t r = 0; r < n; r++)
      for (int64_t p = 0; p < pitch; p++) back[(size_t)(r * pitch + element_at(p))] = b[r * pitch + p];
    CHECK(memcmp(back.data(), nb, (size_t)(n * pitch) * 2) == 0);
  }
  // a row that is no whole number of 32-byte groups is refused, nothing is touched
  std::vector<float> odd(7, 1.f);
  bool threw = false;
  try {
    interleave_h16_rows(odd.data(), 1, 7, 1);
  } catch (std::exception &) {
    threw = true;
  }
  CHECK(threw);
}

int main() {
  check_rule();
  check_rows();
  if (failures) {
    fprintf(stderr, "half_layout_sanitize_test: %d failures\n", failures);
    return 1;
  }
  printf("HALF_LAYOUT_SANITIZE_OK\n");
  return 0;
}
