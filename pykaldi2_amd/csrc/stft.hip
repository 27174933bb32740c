// Short-time Fourier transform and its inverse on the device, float32, hand-written for gfx950: the reference's
// SpectrumAnalyzer (simulation/freq_analysis.py:113-266, stft / istft with center=False), which the ideal-mask estimator
// stands on.
//
//   pk2_stft_f32    frames of `frame_len` samples every `frame_shift`, (x + dither) * window zero-extended to fft_size,
//                   bins 0 .. fft_size / 2; the signal is zero-padded at its end to a whole number of frames
//                   (_enframe(end='pad')).  Output (R, N, F, 2), FRAME-MAJOR (the reference's analyze returns (F, N)).
//   pk2_istft_f32   per frame the inverse real transform (pk2_irfft_pow2_f32 on R * N rows), then overlap-add as a
//                   gather and the division by the summed analysis window.  No synthesis window, as in the reference.
//
// The real transform of length n = fft_size is one complex transform of length h = n / 2 on z[m] = x[2m] + j x[2m+1]
// plus the untangling at its output -- the mirror of what fft.hip does at its input, with the conjugated twiddles of the
// same table:
//   X[k] = (Z[k] + conj Z[h-k]) / 2 - (j / 2) e^{-2 pi j k / n} (Z[k] - conj Z[h-k]),  k = 0 .. h,  Z[h] = Z[0].
// A workgroup owns up to kStftFrames consecutive frames of one row (as many as fit the 4096-point LDS budget: 16 at
// fft_size 512): the contiguous span of the signal they share is staged in LDS once (dither added there), so that
// neighbouring frames do not read HBM again, and their transforms run side by side in lds_fft.
//
// Dither: none; an explicit (R, n) array that is added; or the counter-based generator of sim_rng.h: the pair for
// (row r, sample pair p) is iso_gauss(seed, r * ceil(n / 2) + p), sample 2p takes .x and 2p + 1 takes .y, added as
// x + fl(1e-5f * z) in two rounded steps -- bit-equal to the explicit path fed 1e-5f * pk2_iso_gauss(seed, R, ceil(n / 2)).
#include <algorithm>

#include "common.h"
#include "fft_lds.h"
#include "sim_rng.h"

namespace pk2 {

constexpr int kStftFrames = 16;                 // frames per workgroup at most
constexpr int kStftSpan = 2 * kFftLds;          // floats of staged signal: frames * fft_size <= 8192

struct StftRows {
  const float* x[PK2_SIM_MAX_SEGS];
};

enum { kDitherNone = 0, kDitherArray = 1, kDitherSeed = 2 };

// grid (ceil(N / fb), rows of this launch); row0: index of the launch's first row in the whole call (dither, output)
template <int kDither>
__global__ void __launch_bounds__(kFftThreads) stft_kernel(const StftRows rows, int row0, int64_t n, int nframes, int lgh,
                                                           int frame_len, int frame_shift, int fb,
                                                           const float* __restrict__ window, const float* __restrict__ dither,
                                                           uint64_t seed, const float2* __restrict__ W, float2* __restrict__ out) {
  __shared__ float2 s[kFftLds];
  __shared__ float span[kStftSpan];
  const int h = 1 << lgh;
  const int64_t row = (int64_t)row0 + blockIdx.y;
  const int f0 = blockIdx.x * fb, nf = min(fb, nframes - f0);
  const float* __restrict__ x = rows.x[blockIdx.y];
  const int64_t t0 = (int64_t)f0 * frame_shift;
  const int len = (nf - 1) * frame_shift + frame_len;       // <= fb * fft_size <= kStftSpan
  if (kDither == kDitherSeed) {
    // one draw per sample pair; the span may begin or end in the middle of a pair
    const int64_t p0 = t0 >> 1, p1 = (t0 + len - 1) >> 1, hn = (n + 1) >> 1;
    for (int q = threadIdx.x; q <= (int)(p1 - p0); q += kFftThreads) {
      const int64_t p = p0 + q, t = 2 * p;
      float2 z = make_float2(0.f, 0.f);
      if (t < n) z = iso_gauss(seed, (uint64_t)row * (uint64_t)hn + (uint64_t)p);
      if (t >= t0) span[t - t0] = t < n ? __fadd_rn(x[t], __fmul_rn(1e-5f, z.x)) : 0.f;
      if (t + 1 < t0 + len) span[t + 1 - t0] = t + 1 < n ? __fadd_rn(x[t + 1], __fmul_rn(1e-5f, z.y)) : 0.f;
    }
  } else {
    for (int i = threadIdx.x; i < len; i += kFftThreads) {
      const int64_t t = t0 + i;
      float v = 0.f;
      if (t < n) v = kDither == kDitherArray ? __fadd_rn(x[t], dither[row * n + t]) : x[t];
      span[i] = v;
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < (nf << lgh); idx += kFftThreads) {
    const int b = idx >> lgh, m = idx & (h - 1), i = 2 * m;
    const float* fr = span + b * frame_shift;
    const float v0 = i < frame_len ? fr[i] * window[i] : 0.f;
    const float v1 = i + 1 < frame_len ? fr[i + 1] * window[i + 1] : 0.f;
    s[(b << lgh) + bitrev(m, lgh)] = make_float2(v0, v1);
  }
  lds_fft<true>(s, nf, lgh, W, 2);                  // e^{-2 pi j q / h} = conj W[2 q]
  float2* o = out + (row * nframes + f0) * (int64_t)(h + 1);
  for (int idx = threadIdx.x; idx < nf * (h + 1); idx += kFftThreads) {
    const int b = idx / (h + 1), k = idx - b * (h + 1);
    const float2* Z = s + (b << lgh);
    float2 X;
    if (k == 0 || k == h) {                         // DC and Nyquist: the sums of the even samples +- those of the odd ones
      const float2 z0 = Z[0];
      X = make_float2(k == 0 ? z0.x + z0.y : z0.x - z0.y, 0.f);
    } else {
      const float2 a = Z[k], c = Z[h - k], w = W[k];
      const float2 e = make_float2(a.x + c.x, a.y - c.y), d = make_float2(a.x - c.x, a.y + c.y);      // a +- conj c
      const float2 q = make_float2(d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y);                     // d conj w
      X = make_float2(0.5f * (e.x + q.y), 0.5f * (e.y - q.x));                                        // e / 2 - (j / 2) q
    }
    o[idx] = X;
  }
}

// Overlap-add as a gather: output sample t sums, in frame order, the frames that cover it (at most ceil(fft_size / shift)):
// no atomics, bit-reproducible.  The window sum takes the window's frame_len taps only (freq_analysis.py:202-206); the
// division happens where it exceeds small_float = 1e-10 (:220-221).
__global__ void __launch_bounds__(256) istft_gather_kernel(const float* __restrict__ frames, int nframes, int fft_size,
                                                           int frame_len, int frame_shift, const float* __restrict__ window,
                                                           int64_t L, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= L) return;
  const float* fr = frames + (int64_t)blockIdx.y * nframes * fft_size;
  const int64_t flo = t >= fft_size ? (t - fft_size) / frame_shift + 1 : 0;
  const int64_t fhi = min((int64_t)nframes - 1, t / frame_shift);
  float y = 0.f, ws = 0.f;
  for (int64_t f = flo; f <= fhi; ++f) {
    const int i = (int)(t - f * frame_shift);       // in [0, fft_size)
    y += fr[f * fft_size + i];
    if (i < frame_len) ws += window[i];
  }
  if (ws > 1e-10f) y /= ws;
  out[(int64_t)blockIdx.y * L + t] = y;
}

static int stft_check(const char* who, int32_t fft_size, int32_t frame_len, int32_t frame_shift) {
  PK2_REQUIRE(fft_size >= 32 && fft_size <= 4096 && (fft_size & (fft_size - 1)) == 0,
              "%s: fft_size = %d is not a power of two in [2^5, 2^12]", who, fft_size);
  PK2_REQUIRE(frame_len >= 1 && frame_len <= fft_size, "%s: frame_len = %d is not in [1, fft_size = %d]", who, frame_len, fft_size);
  PK2_REQUIRE(frame_shift >= 1 && frame_shift <= frame_len, "%s: frame_shift = %d is not in [1, frame_len = %d]", who, frame_shift,
              frame_len);
  return PK2_OK;
}

}  // namespace pk2

using namespace pk2;

extern "C" int64_t pk2_stft_num_frames(int64_t n, int32_t frame_len, int32_t frame_shift) {
  if (frame_len < 1 || frame_shift < 1 || n < frame_len) return -1;
  return (n - frame_len + 2 * (int64_t)frame_shift - 1) / frame_shift;
}

extern "C" int pk2_stft_f32(const float* const* rows, int32_t R, int64_t n, int32_t fft_size, int32_t frame_len,
                            int32_t frame_shift, const float* window, const float* dither, int32_t use_seed, uint64_t seed,
                            float* out, void* stream_) {
  PK2_REQUIRE(rows && window && out && R > 0, "stft_f32: null argument or no rows");
  if (int rc = stft_check("stft_f32", fft_size, frame_len, frame_shift)) return rc;
  PK2_REQUIRE(n >= frame_len, "stft_f32: the signal (%lld samples) is shorter than one frame (%d)", (long long)n, frame_len);
  const int64_t N = pk2_stft_num_frames(n, frame_len, frame_shift);
  PK2_REQUIRE(N >= 1 && N <= (1 << 24), "stft_f32: %lld frames (at most 2^24)", (long long)N);
  for (int r = 0; r < R; ++r) PK2_REQUIRE(rows[r], "stft_f32: row %d is null", r);
  const float2* W = nullptr;
  if (int rc = fft_twiddles(fft_size, &W)) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int h = fft_size / 2;
  int lgh = 0;
  while ((1 << lgh) < h) ++lgh;
  const int fb = std::min(kStftFrames, kStftSpan / fft_size);
  const unsigned gx = (unsigned)((N + fb - 1) / fb);
  for (int r0 = 0; r0 < R; r0 += PK2_SIM_MAX_SEGS) {
    const int nr = std::min<int>(PK2_SIM_MAX_SEGS, R - r0);
    StftRows tab;
    for (int r = 0; r < PK2_SIM_MAX_SEGS; ++r) tab.x[r] = r < nr ? rows[r0 + r] : nullptr;
    const dim3 grid(gx, (unsigned)nr);
    float2* o2 = reinterpret_cast<float2*>(out);
    if (dither)
      hipLaunchKernelGGL(stft_kernel<kDitherArray>, grid, dim3(kFftThreads), 0, stream, tab, r0, n, (int)N, lgh, frame_len,
                         frame_shift, fb, window, dither, seed, W, o2);
    else if (use_seed)
      hipLaunchKernelGGL(stft_kernel<kDitherSeed>, grid, dim3(kFftThreads), 0, stream, tab, r0, n, (int)N, lgh, frame_len,
                         frame_shift, fb, window, dither, seed, W, o2);
    else
      hipLaunchKernelGGL(stft_kernel<kDitherNone>, grid, dim3(kFftThreads), 0, stream, tab, r0, n, (int)N, lgh, frame_len,
                         frame_shift, fb, window, dither, seed, W, o2);
    PK2_LAUNCH_CHECK();
  }
  return PK2_OK;
}

extern "C" int pk2_istft_f32(const float* X, int32_t R, int32_t N, int32_t fft_size, int32_t frame_len, int32_t frame_shift,
                             const float* window, float* work, float* out, void* stream_) {
  PK2_REQUIRE(X && window && work && out && R > 0 && R <= 65535 && N > 0 && N <= (1 << 24), "istft_f32: bad arguments");
  if (int rc = stft_check("istft_f32", fft_size, frame_len, frame_shift)) return rc;
  const int64_t rows = (int64_t)R * N, F = fft_size / 2 + 1;
  for (int64_t r0 = 0; r0 < rows; r0 += 65535) {      // (the transform's grid holds 65535 rows)
    const int32_t nr = (int32_t)std::min<int64_t>(65535, rows - r0);
    if (int rc = pk2_irfft_pow2_f32(X + r0 * F * 2, nr, fft_size, work + r0 * fft_size, stream_)) return rc;
  }
  const int64_t L = fft_size + (int64_t)frame_shift * (N - 1);
  hipLaunchKernelGGL(istft_gather_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)R), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), work, N, fft_size, frame_len, frame_shift, window, L, out);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
