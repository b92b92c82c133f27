// wann_bf16.h -- bfloat16 <-> binary32 on the host (portable bit arithmetic, beside wann_half.h).  A bfloat16 is the top 16
// bits of a binary32: every value, subnormals, signed zeros, inf and NaN included, widens exactly by a shift.  binary32 ->
// bfloat16 rounds to nearest, ties to even, on the 16 dropped bits (torch's .to(torch.bfloat16)): magnitudes from 0x7f7f8000
// up round to infinity, infinities stay, a NaN becomes the quiet NaN of its sign.
#pragma once
#include <stdint.h>
#include <string.h>

#include "wann_half.h"
#include "wann_row_types.h"

namespace wann {

inline float bf16_to_float(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

inline uint16_t float_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | 0x7fc0u;         // nan: quiet, sign kept
  const uint32_t r = a + 0x7fffu + ((a >> 16) & 1u);  // nearest, ties to even; the carry walks into the exponent, up to infinity
  return sign | (uint16_t)(r >> 16);
}

// the two-byte float element types (float16, bfloat16) share the row layout; these pick the conversion
inline float two_byte_to_float(int dtype, uint16_t v) { return dtype == kRowsBF16 ? bf16_to_float(v) : half_to_float(v); }
inline uint16_t float_to_two_byte(int dtype, float f) { return dtype == kRowsBF16 ? float_to_bf16(f) : float_to_half(f); }

}  // namespace wann
