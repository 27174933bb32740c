// The LDS-tiled direct-form convolution shared by the single-channel (simulate.hip) and the batched multi-channel
// (simulate_mc.hip) reverberation kernels.
#pragma once
#include "common.h"

namespace pk2 {

constexpr int kSimThreads = 128;
constexpr int kSimOut = 4;                         // outputs per thread
constexpr int kSimTile = kSimThreads * kSimOut;    // outputs per workgroup: small, so that a 12 s utterance makes
                                                   // more workgroups than the GPU has CUs and stagings overlap
constexpr int kSimTaps = 1024;                     // taps staged per pass (4096 FMAs per thread between two barriers)

// 4 taps jj0 .. jj0+3 of the staged pass into the thread's 4 outputs: thread `tid` owns the 4 consecutive outputs
// o = 4 tid + r.  Tap j0 + jj of output o reads s_wav[o + (kSimTaps - 1) - jj]; for the 4 taps the 4 outputs need the
// 7 samples e[0..6] = s_wav[4 tid + 252 - jj0 ...]: two aligned 16-byte LDS reads (conflict-free across lanes) plus
// one broadcast read of the taps feed 16 FMAs.  `ntap` < 4 stops after that many taps (the early-reverberation cut).
template <int ntap>
__device__ __forceinline__ void sim_tile_step(const float* s_rir, const float* s_wav, int tid, int jj0, float (&acc)[kSimOut],
                                              int dyn_taps = 4) {
  const float4 h = *reinterpret_cast<const float4*>(&s_rir[jj0]);
  const float4 lo = *reinterpret_cast<const float4*>(&s_wav[4 * tid + (kSimTaps - 4) - jj0]);
  const float4 hi = *reinterpret_cast<const float4*>(&s_wav[4 * tid + kSimTaps - jj0]);
  const float e[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const float ht[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
  for (int r = 0; r < kSimOut; ++r)
#pragma unroll
    for (int t = 0; t < ntap; ++t)
      if (ntap == 4 || t < dyn_taps) acc[r] = fmaf(ht[t], e[r + 3 - t], acc[r]);
}

// the workgroup's staging buffers (16-byte aligned): declared by the kernel, so that a kernel that instantiates both
// forms of the tile function holds them once
#define PK2_SIM_TILE_LDS                                                     \
  __shared__ __attribute__((aligned(16))) float s_rir[pk2::kSimTaps];        \
  __shared__ __attribute__((aligned(16))) float s_wav[pk2::kSimTile + pk2::kSimTaps]

// out[i] = sum_j rir[j] * wav[i + base - j]  (wav is zero outside [0, n)), outputs [tile * kSimTile, ...) of one row.
// kEarly: early[i] = the same sum over j < cut only, taken as a snapshot of the running sum (0 <= cut <= k): the value
// the full sum has after tap cut - 1, i.e. bit-equal to `out` for the RIR cut to `cut` taps.
template <bool kEarly>
__device__ __forceinline__ void sim_apply_rir_tile(const float* __restrict__ wav, int64_t n, const float* __restrict__ rir,
                                                   int k, int64_t base, float* __restrict__ out, int64_t tile,
                                                   float* s_rir, float* s_wav, float* __restrict__ early = nullptr,
                                                   int cut = 0) {
  const int tid = threadIdx.x;
  const int64_t i0 = tile * kSimTile;
  float acc[kSimOut] = {0.f, 0.f, 0.f, 0.f};
  float snap[kSimOut] = {0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < k; j0 += kSimTaps) {
    const int nt = min(kSimTaps, k - j0);
    // taps j0 .. j0+nt-1 need wav[i0 + base - j0 - (nt-1) .. i0 + kSimTile - 1 + base - j0]
    const int64_t w0 = i0 + base - j0 - (kSimTaps - 1);
    __syncthreads();
    for (int q = tid; q < kSimTaps; q += kSimThreads) s_rir[q] = q < nt ? rir[j0 + q] : 0.f;
    for (int q = tid; q < kSimTile + kSimTaps; q += kSimThreads) {
      const int64_t w = w0 + q;
      s_wav[q] = (w >= 0 && w < n) ? wav[w] : 0.f;
    }
    __syncthreads();
    int jj0 = 0;
    if (kEarly && cut >= j0 && cut < j0 + kSimTaps) {
      // the cut falls into this pass, in general inside a 4-tap step: whole steps up to it, the snapshot with the
      // step's first (cut & 3) taps added, then the pass goes on from that step as if nothing had happened
      const int c4 = (cut - j0) & ~3;
#pragma unroll 4
      for (; jj0 < c4; jj0 += 4) sim_tile_step<4>(s_rir, s_wav, tid, jj0, acc);
#pragma unroll
      for (int r = 0; r < kSimOut; ++r) snap[r] = acc[r];
      sim_tile_step<3>(s_rir, s_wav, tid, c4, snap, (cut - j0) & 3);
    }
#pragma unroll 4
    for (; jj0 < kSimTaps; jj0 += 4) sim_tile_step<4>(s_rir, s_wav, tid, jj0, acc);
  }
  const int64_t i = i0 + 4 * tid;
  // (a row of a (C, n) array starts at a multiple of n floats: 16-byte stores only where the address allows them)
  const bool vec = i + 3 < n && (reinterpret_cast<uintptr_t>(out + i) & 15) == 0 &&
                   (!kEarly || (reinterpret_cast<uintptr_t>(early + i) & 15) == 0);
  if (vec) {
    *reinterpret_cast<float4*>(out + i) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int r = 0; r < kSimOut; ++r)
      if (i + r < n) out[i + r] = acc[r];
  }
  if (kEarly) {
    if (cut >= k) {
#pragma unroll
      for (int r = 0; r < kSimOut; ++r) snap[r] = acc[r];
    }
    if (vec) {
      *reinterpret_cast<float4*>(early + i) = make_float4(snap[0], snap[1], snap[2], snap[3]);
    } else {
#pragma unroll
      for (int r = 0; r < kSimOut; ++r)
        if (i + r < n) early[i + r] = snap[r];
    }
  }
}

}  // namespace pk2
