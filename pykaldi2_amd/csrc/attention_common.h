// What the fused attention kernels of both head sizes share (attention.hip: head size 64, attention128.hip: head size 128):
// the parameter block, the counter-based dropout mask, the additive mask, the 32-wide tiling and its deal to four waves.
#pragma once
#include <cmath>

#include "common.h"

namespace pk2 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kAT = 32;            // tile edge (queries, keys)
constexpr int kAWaves = 4;

struct AttnParams {
  const float* qkv; const float* ctx; const float* dctx; const float* lse_in;
  float* ctx_out; float* lse_out; float* dqkv; float* dsum;
  const float* src_mask; const uint8_t* key_pad; int skip_pad;
  int T, B, H;
  float scale;
  uint32_t keep_threshold; float keep_scale; uint64_t seed; int dropout;
};

// head size 128 (attention128.hip): the launches behind pk2_attention_fwd / pk2_attention_bwd, same grid as head size 64
void attn128_launch_fwd(const AttnParams& p, hipStream_t stream);
void attn128_launch_bwd(const AttnParams& p, int parts, hipStream_t stream);      // parts: bit 0 dQ, bit 1 dK / dV

__device__ __forceinline__ uint32_t attn_mix32(uint64_t z) {     // dropout.hip: splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}
__device__ __forceinline__ float attn_keep(const AttnParams& p, int64_t idx) {
  const uint32_t r = attn_mix32(p.seed * 0xD1342543DE82EF95ull + (uint64_t)idx);
  return r < p.keep_threshold ? p.keep_scale : 0.f;
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tile row the MFMA instruction j reads in the lanes' half hi (see the header of attention.hip)
__device__ __forceinline__ int row_of(int j, int hi) { return (j & 3) + 8 * (j >> 2) + 4 * hi; }

// Additive mask of (query, key): -inf outside the sequence / on padded keys.
__device__ __forceinline__ float mask_of(const AttnParams& p, int b, int q, int k) {
  if (k >= p.T || (p.key_pad && p.key_pad[(int64_t)b * p.T + k])) return -INFINITY;
  return (p.src_mask && q < p.T) ? p.src_mask[(int64_t)q * p.T + k] : 0.f;
}

// Key tiles of utterance b that hold at least one key which is not padding (every wave computes it for itself: T bytes).  The
// tiles behind the last valid key contribute exactly nothing -- every probability is 0 -- and a minibatch of utterances of
// different lengths is mostly such tiles for its short ones (the bench minibatch, 146 / 539 / 569 / 159 frames: 45 of 72
// (utterance, key tile) pairs are valid): the forward and dQ loops end there, a dK / dV workgroup of such a tile stores zeros.
// PK2_ATTN_SKIP_PAD=0 (AttnParams::skip_pad) walks every tile as rounds 2-6a did.
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int valid_key_tiles(const AttnParams& p, int b) {
  const int all = (p.T + kAT - 1) / kAT;
  if (!p.key_pad || !(p.skip_pad & 1)) return all;
  const uint8_t* kp = p.key_pad + (int64_t)b * p.T;
  int last = -1;
  for (int k = threadIdx.x & 63; k < p.T; k += 64)
    if (!kp[k]) last = k;
  last = __builtin_amdgcn_readfirstlane(wave_max_i(last));
  return min(all, (last + kAT) / kAT);
}

}  // namespace pk2
