// Inverse real FFT of power-of-two length (numpy.fft.irfft normalisation), float32, hand-written for gfx950: the last
// step of the isotropic noise generator (reference simulation/_iso_noise_simulator.py:156).
//
// irfft of length n = one complex inverse transform of length h = n / 2 plus the Hermitian untangling at its input:
//   Z[k] = (X[k] + conj X[h-k]) + j (X[k] - conj X[h-k]) e^{2 pi j k / n},   z = IDFT_h(Z),   x[2m] + j x[2m+1] = z[m] / n,
// so the output rows are written as float2.  The complex transform is radix-2 decimation in time in LDS (bit-reversed
// load, one barrier per stage; fft_lds.h).  h <= kFftLds: one workgroup per row.  Beyond that the four-step form h = h1 * h2:
//   pass 1: for every k1 the length-h2 transform over k2 of Z[k1 + h1 k2], times e^{2 pi j k1 m2 / h} -> tmp[k1][m2]
//   pass 2: for every m2 the length-h1 transform over k1 of tmp[k1][m2] -> z[h2 m1 + m2]
// with several columns per workgroup so that global accesses are runs of consecutive elements.  Pass 2 reads and
// writes the same index set per workgroup (all loads before the first store), so tmp is the output array itself.
// Twiddles: one table W[k] = e^{2 pi j k / n}, k < n / 2, computed in float64 on the host and cached per (device, n).
#include <math.h>

#include <map>
#include <mutex>
#include <vector>

#include "common.h"
#include "fft_lds.h"

namespace pk2 {

// Z[k] of the untangling, k in [0, h); X is one row of h + 1 complex bins
__device__ __forceinline__ float2 untangle(const float2* __restrict__ X, int k, int h, const float2* __restrict__ W) {
  float2 a = X[k], b = X[h - k];
  if (k == 0) { a.y = 0.f; b.y = 0.f; }            // numpy ignores the imaginary parts of DC and Nyquist
  const float2 e = make_float2(a.x + b.x, a.y - b.y), d = make_float2(a.x - b.x, a.y + b.y);     // a +- conj b
  const float2 w = W[k];
  const float2 o = make_float2(d.x * w.x - d.y * w.y, d.x * w.y + d.y * w.x);
  return make_float2(e.x - o.y, e.y + o.x);
}

// h <= kFftLds: one workgroup per row
__global__ void __launch_bounds__(kFftThreads) irfft_lds_kernel(const float2* __restrict__ X, int lgh, const float2* __restrict__ W,
                                                                float2* __restrict__ out) {
  __shared__ float2 s[kFftLds];
  const int h = 1 << lgh;
  const float2* Xr = X + (int64_t)blockIdx.x * (h + 1);
  for (int k = threadIdx.x; k < h; k += kFftThreads) s[bitrev(k, lgh)] = untangle(Xr, k, h, W);
  lds_fft(s, 1, lgh, W, 2);                         // e^{2 pi j q / h} = W[2 q]
  const float inv = 1.f / (float)(2 * h);
  float2* o = out + (int64_t)blockIdx.x * h;
  for (int m = threadIdx.x; m < h; m += kFftThreads) o[m] = make_float2(s[m].x * inv, s[m].y * inv);
}

// pass 1 of the four-step form: workgroup (x, row) owns the columns k1 in [x * B, (x + 1) * B), B = kFftLds / h2
__global__ void __launch_bounds__(kFftThreads) irfft_pass1_kernel(const float2* __restrict__ X, int lgh, int lg1, const float2* __restrict__ W,
                                                                  float2* __restrict__ tmp) {
  __shared__ float2 s[kFftLds];
  const int lg2 = lgh - lg1, h = 1 << lgh, h1 = 1 << lg1, h2 = 1 << lg2;
  const int lgB = min(12 - lg2, lg1), B = 1 << lgB;
  const int k10 = blockIdx.x << lgB;
  const float2* Xr = X + (int64_t)blockIdx.y * (h + 1);
  for (int t = threadIdx.x; t < (B << lg2); t += kFftThreads) {
    const int b = t & (B - 1), k2 = t >> lgB;      // consecutive threads: consecutive k1
    s[(b << lg2) + bitrev(k2, lg2)] = untangle(Xr, k10 + b + (k2 << lg1), h, W);
  }
  lds_fft(s, B, lg2, W, 2 * h1);                    // e^{2 pi j q / h2} = W[q * n / h2] = W[2 h1 q]
  float2* tr = tmp + (int64_t)blockIdx.y * h;
  for (int t = threadIdx.x; t < (B << lg2); t += kFftThreads) {
    const int b = t >> lg2, m2 = t & (h2 - 1);
    const int k1 = k10 + b;
    // e^{2 pi j k1 m2 / h} = W[2 k1 m2]; 2 k1 m2 < n, and W[q + h] = -W[q]
    const int q = 2 * k1 * m2;
    float2 w = W[q & (h - 1)];
    if (q & h) { w.x = -w.x; w.y = -w.y; }
    const float2 v = s[t];
    tr[((int64_t)k1 << lg2) + m2] = make_float2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
  }
}

// pass 2: workgroup (x, row) owns the columns m2 in [x * B, (x + 1) * B), B = kFftLds / h1; in place
__global__ void __launch_bounds__(kFftThreads) irfft_pass2_kernel(int lgh, int lg1, const float2* __restrict__ W, float2* io) {
  __shared__ float2 s[kFftLds];
  const int lg2 = lgh - lg1, h = 1 << lgh, h2 = 1 << lg2;
  const int lgB = min(12 - lg1, lg2), B = 1 << lgB;
  const int m20 = blockIdx.x << lgB;
  float2* r = io + (int64_t)blockIdx.y * h;
  for (int t = threadIdx.x; t < (B << lg1); t += kFftThreads) {
    const int b = t & (B - 1), k1 = t >> lgB;
    s[(b << lg1) + bitrev(k1, lg1)] = r[((int64_t)k1 << lg2) + m20 + b];
  }
  lds_fft(s, B, lg1, W, 2 * h2);                    // e^{2 pi j q / h1} = W[2 h2 q]
  const float inv = 1.f / (float)(2 * h);
  for (int t = threadIdx.x; t < (B << lg1); t += kFftThreads) {
    const int b = t & (B - 1), m1 = t >> lgB;
    const float2 v = s[(b << lg1) + m1];
    r[((int64_t)m1 << lg2) + m20 + b] = make_float2(v.x * inv, v.y * inv);
  }
}

struct TwiddleKey {
  int dev, n;
  bool operator<(const TwiddleKey& o) const { return dev != o.dev ? dev < o.dev : n < o.n; }
};
static std::mutex g_tw_mutex;
static std::map<TwiddleKey, float2*> g_tw;

// W[k] = e^{2 pi j k / n}, k < n / 2: float64 on the host, one blocking upload the first time a length is used
int fft_twiddles(int n, const float2** out) {
  std::lock_guard<std::mutex> lock(g_tw_mutex);
  const TwiddleKey key{current_device(), n};
  auto it = g_tw.find(key);
  if (it == g_tw.end()) {
    const int h = n / 2;
    std::vector<float2> host(h);
    for (int k = 0; k < h; ++k) {
      const double a = 2.0 * M_PI * (double)k / (double)n;
      host[k] = make_float2((float)cos(a), (float)sin(a));
    }
    float2* dev = nullptr;
    PK2_HIP(hipMalloc(&dev, sizeof(float2) * h));
    PK2_HIP(hipMemcpy(dev, host.data(), sizeof(float2) * h, hipMemcpyHostToDevice));
    it = g_tw.emplace(key, dev).first;
  }
  *out = it->second;
  return PK2_OK;
}

}  // namespace pk2

using namespace pk2;

extern "C" int pk2_irfft_pow2_f32(const float* X, int32_t rows, int32_t n, float* out, void* stream_) {
  PK2_REQUIRE(X && out && rows > 0 && rows <= 65535, "irfft_pow2_f32: bad arguments");
  PK2_REQUIRE(n >= 32 && n <= (1 << 20) && (n & (n - 1)) == 0, "irfft_pow2_f32: n = %d is not a power of two in [2^5, 2^20]", n);
  PK2_REQUIRE(X != out, "irfft_pow2_f32: in-place operation is not supported");
  const float2* W = nullptr;
  if (int rc = fft_twiddles(n, &W)) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int h = n / 2;
  int lgh = 0;
  while ((1 << lgh) < h) ++lgh;
  const float2* X2 = reinterpret_cast<const float2*>(X);
  float2* o2 = reinterpret_cast<float2*>(out);
  if (h <= kFftLds) {
    hipLaunchKernelGGL(irfft_lds_kernel, dim3((unsigned)rows), dim3(kFftThreads), 0, stream, X2, lgh, W, o2);
    PK2_LAUNCH_CHECK();
    return PK2_OK;
  }
  const int lg1 = lgh / 2, lg2 = lgh - lg1;         // h <= 2^19: lg1 <= 9, lg2 <= 10, both transforms fit LDS several at a time
  const int lgB1 = std::min(12 - lg2, lg1), lgB2 = std::min(12 - lg1, lg2);
  hipLaunchKernelGGL(irfft_pass1_kernel, dim3(1u << (lg1 - lgB1), (unsigned)rows), dim3(kFftThreads), 0, stream, X2, lgh, lg1, W, o2);
  PK2_LAUNCH_CHECK();
  hipLaunchKernelGGL(irfft_pass2_kernel, dim3(1u << (lg2 - lgB2), (unsigned)rows), dim3(kFftThreads), 0, stream, lgh, lg1, W, o2);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
