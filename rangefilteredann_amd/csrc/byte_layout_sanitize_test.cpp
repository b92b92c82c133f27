// byte_layout_sanitize_test.cpp -- the layout of the device copy of the one-byte shadow rows (u8_row_position in wann_row_types.h,
// interleave_u8_rows in wann_build.cpp) under address + undefined-behaviour sanitizers (make sanitize): the packed rows of a
// point set, interleaved in buffers of exactly n rows, hold x[r][e] at byte u8_row_position(e) of row r and zero in every other
// byte, and the permutation's inverse gives the packed rows back.  CPU only; no HIP.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <stdexcept>
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

// the element stored at byte `pos` of a row: the inverse of u8_row_position, written out on its own
static int64_t element_at(int64_t pos) {
  const int64_t r = pos & 31;
  return 32 * (pos >> 5) + 8 * ((r >> 2) & 3) + 4 * ((r >> 4) & 1) + (r & 3);
}

// the rule itself: a permutation of every aligned group of 32, quads of lane h's blocks contiguous and in order
static void check_rule() {
  static_assert(u8_row_position(0) == 0 && u8_row_position(3) == 3 && u8_row_position(4) == 16 && u8_row_position(8) == 4 &&
                    u8_row_position(12) == 20 && u8_row_position(31) == 31 && u8_row_position(32) == 32 && u8_row_position(36) == 48,
                "the interleaved layout");
  for (int64_t e = 0; e < 4096; e++) {
    const int64_t p = u8_row_position(e);
    CHECK(p == 32 * (e >> 5) + 16 * ((e >> 2) & 1) + 4 * ((e >> 3) & 3) + (e & 3));
    CHECK((p >> 5) == (e >> 5));
    CHECK(element_at(p) == e);
  }
  for (int64_t c = 0; c < 128; c++)
    for (int64_t h = 0; h < 2; h++)
      for (int64_t i = 0; i < 4; i++)
        for (int64_t j = 0; j < 4; j++) CHECK(u8_row_position(8 * (4 * c + i) + 4 * h + j) == 32 * c + 16 * h + 4 * i + j);
}

static void check_rows() {
  const int64_t dims[] = {1, 20, 32, 33, 64, 65, 100, 128, 136, 200, 264};
  for (int64_t d : dims) {
    const int64_t n = 37, stride = (d + 15) / 16 * 16, words = u8_widened_stride_words(d), pitch = words * 4;
    CHECK(pitch % 32 == 0 && pitch >= d);
    std::vector<float> pts((size_t)(n * stride), 0.f);
    for (int64_t r = 0; r < n; r++)
      for (int64_t e = 0; e < d; e++) pts[(size_t)(r * stride + e)] = (float)(1 + (r * 31 + e * 17 + 128) % 255);  // (never 0: a value in a padding byte shows)
    CHECK(rows_u8_exact(pts.data(), n, d, stride, 3));
    std::vector<float> packed((size_t)(n * words), 0.f);  // (exactly n rows: an access past the last row is the sanitizer's to find)
    pack_u8_rows(pts.data(), n, d, stride, words, 3, packed.data());
    std::vector<float> rows(packed);
    interleave_u8_rows(rows.data(), n, words, 3);
    const uint8_t *b = reinterpret_cast<const uint8_t *>(rows.data());
    const uint8_t *nat = reinterpret_cast<const uint8_t *>(packed.data());
    bool values = true, zeros = true, inverse = true;
    std::vector<uint8_t> owned((size_t)pitch);
    for (int64_t r = 0; r < n; r++) {
      std::fill(owned.begin(), owned.end(), (uint8_t)0);
      for (int64_t e = 0; e < d; e++) {
        const int64_t p = u8_row_position(e);
        if (p < 0 || p >= pitch) {
          values = false;
          continue;
        }
        owned[(size_t)p] = 1;
        values = values && (float)b[r * pitch + p] == pts[(size_t)(r * stride + e)];
      }
      for (int64_t p = 0; p < pitch; p++) {
        if (!owned[(size_t)p]) zeros = zeros && b[r * pitch + p] == 0;
        inverse = inverse && b[r * pitch + p] == nat[r * pitch + element_at(p)];
      }
    }
    CHECK(values);
    CHECK(zeros);
    CHECK(inverse);
    // ... and undone byte by byte, the packed rows again
    std::vector<uint8_t> back((size_t)(n * pitch));
    for (int64_t r = 0; r < n; r++)
      for (int64_t p = 0; p < pitch; p++) back[(size_t)(r * pitch + element_at(p))] = b[r * pitch + p];
    CHECK(memcmp(back.data(), nat, (size_t)(n * pitch)) == 0);
  }
  // the C ABI's function is the same rule
  for (int64_t e = 0; e < 4096; e++) CHECK(u8_row_position(e) == 32 * (e / 32) + u8_row_position(e % 32));
  // a row that is no whole number of 32-byte groups is refused, nothing is touched
  std::vector<float> odd(7, 1.f);
  bool threw = false;
  try {
    interleave_u8_rows(odd.data(), 1, 7, 1);
  } catch (std::exception &) {
    threw = true;
  }
  CHECK(threw);
}

int main() {
  check_rule();
  check_rows();
  if (failures) {
    fprintf(stderr, "byte_layout_sanitize_test: %d failures\n", failures);
    return 1;
  }
  printf("BYTE_LAYOUT_SANITIZE_OK\n");
  return 0;
}
