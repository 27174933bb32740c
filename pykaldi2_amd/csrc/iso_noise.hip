// Isotropic (spherically / cylindrically diffuse) noise field for a microphone array in the frequency domain: the sum
// over 512 plane-wave directions of the reference's generate_isotropic_noise (simulation/_iso_noise_simulator.py:97-160,
// after Habets & Gannot, JASA 122(6), 2007), which numpy runs at ~10 s for a 10 s utterance -- the reason the
// reference's configs fall back to a noise corpus.
//
//   pk2_iso_spectra   X[m][f] = (1/sqrt(P)) sum_i g[f] Z_i[f] exp(-j tau[m][i] w_f) with the reference's bin scaling
//   pk2_iso_gauss     the draws Z of the built-in generator (sim_rng.h; tests and tools)
// One thread owns one frequency bin of up to kIsoMics microphones and walks the directions in order: no atomics, the
// result is bit-reproducible.  tau[m][i] is uniform over the workgroup (scalar loads); the phase tau * f / fft_size is
// reduced to [-1/2, 1/2] turns in float64 (it reaches hundreds of radians for a large array) before the float32 sincospi.
#include <algorithm>

#include "common.h"
#include "sim_rng.h"

namespace pk2 {

constexpr int kIsoMics = 4;          // microphones per thread: the draw (hash, log, sqrt, sincospi) is shared by them

template <bool kDraws>
__global__ void __launch_bounds__(256) iso_spectra_kernel(const double* __restrict__ tau, const double* __restrict__ g,
                                                          const float2* __restrict__ draws, uint64_t seed, int channels,
                                                          int points, int bins, float2* __restrict__ X) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= bins) return;
  const int m0 = blockIdx.y * kIsoMics;
  const int fft_size = 2 * (bins - 1);
  const double turn = (double)f / (double)fft_size;        // w_f / (2 pi), exact
  const float gf = g ? (float)g[f] : 1.f;
  float re[kIsoMics], im[kIsoMics];
#pragma unroll
  for (int q = 0; q < kIsoMics; ++q) re[q] = im[q] = 0.f;
  for (int i = 0; i < points; ++i) {
    float2 z = kDraws ? draws[(int64_t)i * bins + f] : iso_gauss(seed, (uint64_t)i * (uint64_t)bins + (uint64_t)f);
    z.x *= gf;
    z.y *= gf;
#pragma unroll
    for (int q = 0; q < kIsoMics; ++q) {
      const int m = min(m0 + q, channels - 1);              // the spare slots of the last group repeat its last microphone
      double ph = tau[(int64_t)m * points + i] * turn;
      ph -= rint(ph);
      float s, c;
      sincospif(-2.f * (float)ph, &s, &c);                  // exp(-j tau w)
      re[q] = fmaf(z.x, c, fmaf(-z.y, s, re[q]));
      im[q] = fmaf(z.x, s, fmaf(z.y, c, im[q]));
    }
  }
  // X / sqrt(P), then (:152-154) DC and Nyquist -> sqrt(fft_size) Re, the others * sqrt(fft_size / 2)
  const float inv = (float)(1.0 / sqrt((double)points));
  const bool edge = f == 0 || f == bins - 1;
  const float sc = (float)(edge ? sqrt((double)fft_size) : sqrt((double)(fft_size / 2)));
#pragma unroll
  for (int q = 0; q < kIsoMics; ++q) {
    const int m = m0 + q;
    if (m < channels) X[(int64_t)m * bins + f] = make_float2(re[q] * inv * sc, edge ? 0.f : im[q] * inv * sc);
  }
}

__global__ void __launch_bounds__(256) iso_gauss_kernel(uint64_t seed, int64_t total, float2* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    out[i] = iso_gauss(seed, (uint64_t)i);
}

}  // namespace pk2

using namespace pk2;

extern "C" int pk2_iso_spectra(const double* tau, const double* g, const float* draws, uint64_t seed, int32_t channels,
                               int32_t points, int32_t bins, float* X, void* stream_) {
  PK2_REQUIRE(tau && X && channels > 0 && channels <= 65535 * kIsoMics && points > 0 && bins >= 2 && bins <= (1 << 24) + 1,
              "iso_spectra: bad arguments");
  PK2_REQUIRE(((bins - 1) & (bins - 2)) == 0, "iso_spectra: %d bins are not fft_size / 2 + 1 of a power-of-two FFT", bins);
  const dim3 grid((unsigned)((bins + 255) / 256), (unsigned)((channels + kIsoMics - 1) / kIsoMics));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (draws)
    hipLaunchKernelGGL(iso_spectra_kernel<true>, grid, dim3(256), 0, stream, tau, g, reinterpret_cast<const float2*>(draws), seed,
                       channels, points, bins, reinterpret_cast<float2*>(X));
  else
    hipLaunchKernelGGL(iso_spectra_kernel<false>, grid, dim3(256), 0, stream, tau, g, static_cast<const float2*>(nullptr), seed,
                       channels, points, bins, reinterpret_cast<float2*>(X));
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_iso_gauss(uint64_t seed, int32_t points, int32_t bins, float* out, void* stream_) {
  PK2_REQUIRE(out && points > 0 && bins > 0, "iso_gauss: bad arguments");
  const int64_t total = (int64_t)points * bins;
  hipLaunchKernelGGL(iso_gauss_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), seed, total, reinterpret_cast<float2*>(out));
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
