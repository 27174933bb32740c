// Counter-based normal draws of the simulation kernels: the isotropic noise field (iso_noise.hip) and the STFT's dither
// (stft.hip).  A draw is a pure function of (seed, counter), so a kernel may make it wherever it is needed and
// pk2_iso_gauss writes out the very same numbers.
#pragma once
#include "common.h"

namespace pk2 {

// splitmix64 finaliser (the one of dropout.hip), all 64 bits
__device__ __forceinline__ uint64_t iso_mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// One complex standard normal, a pure function of (seed, counter): u1, u2 = (k + 0.5) 2^-24 from bits 63..40 and 39..16,
// Box-Muller.  k + 0.5 has 25 significant bits; for k >= 2^23 float32 would round u1 (to 1.0 for the last k), so the
// logarithm of the upper half is taken as log1p(-(2^24 - k - 0.5) 2^-24), whose argument is exact.
__device__ __forceinline__ float2 iso_gauss(uint64_t seed, uint64_t counter) {
  const uint64_t z = iso_mix64(seed * 0xD1342543DE82EF95ull + counter);
  const uint32_t k1 = (uint32_t)(z >> 40), k2 = (uint32_t)(z >> 16) & 0xFFFFFFu;
  const float lg = k1 < (1u << 23) ? logf(((float)k1 + 0.5f) * 0x1p-24f)
                                   : log1pf(-((float)((1u << 24) - 1u - k1) + 0.5f) * 0x1p-24f);
  const float r = sqrtf(-2.f * lg);
  float s, c;
  sincospif(((float)k2 + 0.5f) * 0x1p-23f, &s, &c);       // angle 2 pi u2; (k2 + 0.5) 2^-23 is rounded harmlessly
  return make_float2(r * c, r * s);
}

}  // namespace pk2
