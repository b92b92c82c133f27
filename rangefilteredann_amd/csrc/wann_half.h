// wann_half.h -- IEEE binary16 <-> binary32 on the host (portable bit arithmetic: the host objects are built by compilers
// without a _Float16 type).  Every binary16 value, subnormals and signed zeros included, converts to binary32 exactly;
// binary32 -> binary16 rounds to nearest, ties to even (numpy's astype(np.float16)).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace wann {

inline float half_to_float(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t u;
  if (e == 0x1f) {
    u = sign | 0x7f800000u | (m << 13);  // inf / nan
  } else if (e != 0) {
    u = sign | ((e + 112) << 23) | (m << 13);
  } else {
    const float f = (float)m * 0x1p-24f;  // subnormal (or zero): m * 2^-24, exact
    memcpy(&u, &f, 4);
    u |= sign;
  }
  float f;
  memcpy(&f, &u, 4);
  return f;
}

inline uint16_t float_to_half(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const uint32_t a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u);  // inf / nan
  if (a >= 0x477ff000u) return sign | 0x7c00u;                                       // rounds to infinity (>= 65520)
  if (a < 0x38800000u) {                                                               // below 2^-14: a subnormal half
    float v;
    memcpy(&v, &a, 4);
    return sign | (uint16_t)nearbyintf(v * 0x1p24f);  // exact scaling, then the current (nearest-even) rounding
  }
  const uint32_t r = a + 0xfffu + ((a >> 13) & 1u);  // nearest, ties to even, on the 13 dropped bits
  return sign | (uint16_t)((r - 0x38000000u) >> 13);
}

}  // namespace wann
