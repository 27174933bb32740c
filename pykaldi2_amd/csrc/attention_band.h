// What the banded attention kernels (attention_band.hip) share between head sizes 64 and 128: the band and its interval
// arithmetic, and the tile helpers of attention.hip / attention128.hip written once over the head size, with the staging
// done by a whole workgroup instead of a wave.
#pragma once
#include "attention_common.h"

namespace pk2 {

// Query q sees key k iff  lo(q) <= k <= hi(q),  lo(q) = left < 0 ? 0 : c(q) - left,  hi(q) = right < 0 ? T - 1 :
// c(q) + chunk - 1 + right,  c(q) = q / chunk * chunk (and k < T, key k not padded).  The host clamps left, right and chunk
// to T, which changes no interval and keeps every sum below inside int32.
struct Band { int left, right, chunk; };

__device__ __forceinline__ int band_key_lo(const Band& bd, int q) {
  return bd.left < 0 ? 0 : max(0, q / bd.chunk * bd.chunk - bd.left);
}
__device__ __forceinline__ int band_key_hi(const Band& bd, int q, int T) {
  return bd.right < 0 ? T - 1 : min(T - 1, q / bd.chunk * bd.chunk + bd.chunk - 1 + bd.right);
}
// The inverse: the queries that see key k are the interval [band_query_lo, band_query_hi], because lo() and hi() do not
// decrease with q.  Its ends are chunk ends: the first query is the first of the first chunk j with j chunk + chunk - 1 +
// right >= k, the last query the last of the last chunk j with j chunk - left <= k.
__device__ __forceinline__ int band_query_lo(const Band& bd, int k) {
  if (bd.right < 0) return 0;
  const int x = k - bd.chunk + 1 - bd.right;                     // j chunk >= x
  return x <= 0 ? 0 : (x + bd.chunk - 1) / bd.chunk * bd.chunk;
}
__device__ __forceinline__ int band_query_hi(const Band& bd, int k, int T) {
  return bd.left < 0 ? T - 1 : min(T - 1, (k + bd.left) / bd.chunk * bd.chunk + bd.chunk - 1);
}

// bit i <-> element base + i of a 32-wide tile: set for the elements inside [a, b]
__device__ __forceinline__ uint32_t interval_bits(int a, int b, int base) {
  const int lo = max(a - base, 0), hi = min(b - base, kAT - 1);
  return lo > hi ? 0u : (0xFFFFFFFFu >> (kAT - 1 - hi)) & (0xFFFFFFFFu << lo);
}

constexpr int kBRing = 2;          // staged tile pairs of a workgroup (see the header of attention_band.hip)
constexpr int kBThreads = 64 * kAWaves;

// Tile helpers over the head size D; NT = the threads that stage a tile together (a wave or the workgroup).
template <int D>
struct BandTile {
  static constexpr int kLd = D + 1;            // LDS row pitch: rows on different banks
  static constexpr int kFloats = kAT * kLd;
  static constexpr int kNR = D / 2;            // registers of a row operand = MFMA instructions of a row product
  static constexpr int kNB = D / 32;           // 32-dim blocks of a transposed accumulator
  // dim the MFMA instruction i of a row product contracts in the lanes' half hi, relative to 32 hi (attention128.hip)
  __device__ static __forceinline__ int dim_of(int i) { return (i & 31) + 64 * (i >> 5); }

  template <int NT> struct Regs { float4 v[kAT * D / 4 / NT]; };
  // rows [r0, r0 + 32) of a matrix with row stride rs, D columns from base; rows >= T read as zero (no branch per row:
  // attention128.hip, fetch_tile).  t = this thread's index among the NT.
  template <int NT>
  __device__ static __forceinline__ void fetch(const float* __restrict__ base, int64_t rs, int r0, int T, int t, Regs<NT>& x) {
#pragma unroll
    for (int it = 0; it < kAT * D / 4 / NT; ++it) {
      const int idx = it * NT + t, row = idx / (D / 4), col = idx % (D / 4) * 4;
      const float4 v = *reinterpret_cast<const float4*>(base + (int64_t)min(r0 + row, T - 1) * rs + col);
      const uint32_t keep = r0 + row < T ? 0xFFFFFFFFu : 0u;
      x.v[it] = make_float4(__uint_as_float(__float_as_uint(v.x) & keep), __uint_as_float(__float_as_uint(v.y) & keep),
                            __uint_as_float(__float_as_uint(v.z) & keep), __uint_as_float(__float_as_uint(v.w) & keep));
    }
  }
  template <int NT>
  __device__ static __forceinline__ void put(const Regs<NT>& x, float* tile, int t, float s = 1.0f) {
#pragma unroll
    for (int it = 0; it < kAT * D / 4 / NT; ++it) {
      const int idx = it * NT + t;
      float* o = tile + idx / (D / 4) * kLd + idx % (D / 4) * 4;
      o[0] = x.v[it].x * s; o[1] = x.v[it].y * s; o[2] = x.v[it].z * s; o[3] = x.v[it].w * s;
    }
  }
  // One wave's 32 rows from global memory into its "row operand" registers, through a tile of its own:
  // lane (row = lane % 32, hi = lane / 32) -> s * M[r0 + row][32 hi + dim_of(i)], i < kNR
  __device__ static __forceinline__ void load_rows(const float* __restrict__ base, int64_t rs, int r0, int T, float* tile,
                                                   float s, float (&r)[kNR]) {
    const int lane = threadIdx.x & 63;
    {
      Regs<64> x;
      fetch<64>(base, rs, r0, T, lane, x);
      put<64>(x, tile, lane, s);
    }
    wave_lds_sync();
    const float* src = tile + (lane & 31) * kLd + 32 * (lane >> 5);
#pragma unroll
    for (int i = 0; i < kNR; ++i) r[i] = src[dim_of(i)];
    wave_lds_sync();
  }
  // acc[row][n] = sum_dim tile[row][dim] * b[dim][n], b = a row operand of the n side
  __device__ static __forceinline__ f32x16 mfma_rows(const float* tile, const float (&b)[kNR]) {
    const int lane = threadIdx.x & 63;
    const float* src = tile + (lane & 31) * kLd + 32 * (lane >> 5);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < kNR; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(src[dim_of(i)], b[i], acc, 0, 0, 0);
    return acc;
  }
  // acc[dim][n] += sum_rows tile[row][dim] * w[row][n], w an accumulator-layout register set (register j <-> rows row_of(j, hi))
  __device__ static __forceinline__ void mfma_tile_t(const float* tile, const f32x16& w, f32x16 (&acc)[kNB]) {
    const int lane = threadIdx.x & 63, hi = lane >> 5, m = lane & 31;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float* src = tile + row_of(j, hi) * kLd + m;
#pragma unroll
      for (int c = 0; c < kNB; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[32 * c], w[j], acc[c], 0, 0, 0);
    }
  }
  __device__ static __forceinline__ void zero_acc(f32x16 (&acc)[kNB]) {
#pragma unroll
    for (int c = 0; c < kNB; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  }
  // a lane's dims 32 c + 8 g + 4 hi + (0..3) of its row -> out_row[...], scaled
  __device__ static __forceinline__ void store_t(float* out_row, int hi, const f32x16 (&acc)[kNB], float s) {
#pragma unroll
    for (int c = 0; c < kNB; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(out_row + 32 * c + 8 * g + 4 * hi) =
            make_float4(acc[c][4 * g] * s, acc[c][4 * g + 1] * s, acc[c][4 * g + 2] * s, acc[c][4 * g + 3] * s);
  }
};
}  // namespace pk2
