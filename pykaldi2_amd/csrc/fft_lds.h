// In-LDS radix-2 transform shared by the inverse real FFT (fft.hip) and the forward STFT (stft.hip), and the twiddle
// table both read: W[k] = e^{2 pi j k / n}, k < n / 2, computed in float64 on the host and cached per (device, n).
// The inverse direction multiplies by W, the forward one by its conjugate.
#pragma once
#include "common.h"

namespace pk2 {

constexpr int kFftLds = 4096;        // complex points in LDS (32 KB)
constexpr int kFftThreads = 256;

// In-LDS radix-2 DIT on `nb` independent transforms of `len` = 1 << lg points each, s[b * len + bitrev(index)] loaded
// by the caller.  W[q * wstride] = e^{2 pi j q / len}; kConj: the forward transform (twiddles e^{-2 pi j q / len}).
// Ends with a barrier.
template <bool kConj = false>
__device__ __forceinline__ void lds_fft(float2* s, int nb, int lg, const float2* __restrict__ W, int wstride) {
  const int len = 1 << lg, half = (nb << lg) >> 1;
  for (int st = 0; st < lg; ++st) {
    const int m = 1 << st;
    __syncthreads();
    for (int t = threadIdx.x; t < half; t += kFftThreads) {
      const int b = t >> (lg - 1), u = t & ((len >> 1) - 1);
      const int j = u & (m - 1);
      const int i0 = (b << lg) + ((u - j) << 1) + j, i1 = i0 + m;
      float2 w = W[(int64_t)j * (len >> (st + 1)) * wstride];
      if (kConj) w.y = -w.y;
      const float2 a = s[i0], c = s[i1];
      const float2 p = make_float2(c.x * w.x - c.y * w.y, c.x * w.y + c.y * w.x);
      s[i0] = make_float2(a.x + p.x, a.y + p.y);
      s[i1] = make_float2(a.x - p.x, a.y - p.y);
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int bitrev(int x, int lg) { return (int)(__brev((unsigned)x) >> (32 - lg)); }

// W of length n (a power of two) on the current device: one blocking upload the first time a length is used (fft.hip)
int fft_twiddles(int n, const float2** out);

}  // namespace pk2
