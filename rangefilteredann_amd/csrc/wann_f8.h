// wann_f8.h -- float8 (OCP E4M3, "e4m3fn") <-> binary32 on the host (portable bit arithmetic, table-free, beside wann_half.h and
// wann_bf16.h).  A pattern is 1 sign bit, 4 exponent bits with bias 7 and 3 mantissa bits; there are no infinities, 0x7f / 0xff
// are NaN, the largest finite value is 448 (0x7e), subnormals are M * 2^-9.  Every finite pattern widens exactly: four
// significant bits, exponents 2^-9 .. 2^8 -- all normal binary32 (and bfloat16) values.
// binary32 -> float8 rounds the VALUE to nearest, ties to even (torch's .to(torch.float8_e4m3fn)): a magnitude that rounds above
// 448 becomes the NaN pattern of its sign, and so do the infinities and NaN -- 464 ties down to 448, anything larger is NaN;
// 2^-10 ties down to zero.  Nothing saturates: the index refuses NaN patterns (f8_first_nan_row), so out-of-range data is an error.
#pragma once
#include <stdint.h>
#include <string.h>

namespace wann {

constexpr bool f8_is_nan(uint8_t b) { return (b & 0x7fu) == 0x7fu; }

inline float f8_to_float(uint8_t b) {
  const uint32_t sign = (uint32_t)(b & 0x80u) << 24, e = (b >> 3) & 15u, m = b & 7u;
  uint32_t u;
  if (e == 15u && m == 7u) {
    u = sign | 0x7fc00000u;  // nan: quiet, sign kept
  } else if (e == 0u) {
    if (m == 0u) {
      u = sign;  // signed zero
    } else {     // subnormal M * 2^-9: the leading bit of M becomes the hidden bit
      const uint32_t p = m >= 4u ? 2u : m >= 2u ? 1u : 0u;
      u = sign | ((127u - 9u + p) << 23) | ((m << (23u - p)) & 0x7fffffu);
    }
  } else {
    u = sign | ((e - 7u + 127u) << 23) | (m << 20);
  }
  float f;
  memcpy(&f, &u, 4);
  return f;
}

inline uint8_t float_to_f8(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
  const uint32_t a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return sign | 0x7fu;  // inf, nan
  const uint32_t exp32 = a >> 23;
  if (exp32 >= 121u) {  // |f| >= 2^-6: a normal float8, or beyond the range
    // nearest, ties to even, on the 20 dropped bits; the carry walks into the exponent
    const uint32_t r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;  // float32 exponent << 3 | three mantissa bits
    const uint32_t code = r - ((127u - 7u) << 3);
    return sign | (uint8_t)(code >= 0x7fu ? 0x7fu : code);  // rounds above 448: the NaN pattern
  }
  // |f| < 2^-6: M = |f| * 2^9 rounded to an integer 0 .. 8 (8 is the code of 2^-6, the smallest normal)
  const uint32_t shift = 141u - exp32;  // M = sig >> shift, sig the 24-bit significand; >= 21 here
  if (exp32 == 0u || shift >= 25u) return sign;  // below 2^-10 (float32 subnormals included): zero
  const uint32_t sig = (a & 0x7fffffu) | 0x800000u;
  const uint32_t M = (sig + (1u << (shift - 1u)) - 1u + ((sig >> shift) & 1u)) >> shift;
  return sign | (uint8_t)M;
}

// the first row of an (n, d) array of float8 patterns that holds a NaN pattern; -1: none
inline int64_t f8_first_nan_row(const uint8_t *p, int64_t n, int64_t d) {
  for (int64_t i = 0, count = n * d; i < count; i++)
    if (f8_is_nan(p[i])) return i / d;
  return -1;
}

}  // namespace wann
