// Fused multi-head self-attention for gfx950 at head size 128 (f32 MFMA): the kernels behind pk2_attention_fwd / _bwd for
// the transformer command lines' default -dim_model 512 -nheads 4.  Same contract, same 32 x 32 (query x key) tiles on
// v_mfma_f32_32x32x2_f32, same transposed layout and same deal of tiles to four waves as attention.hip (read its header
// first); what differs is what a head twice as wide does to the register file and to LDS:
//
//   * one workgroup per CU, one wave per SIMD: a wave may use all 512 registers (256 VGPRs + 256 AGPRs).  The row operands
//     (Q, dO, or K, V) are 64 registers each, the transposed accumulators (O, dQ, or dK, dV) 64 each.
//   * two [32][129] tiles per wave are 33 KB, 132 KB per workgroup of the CU's 160 KB.
//   * the dims of a head are dealt to the MFMA's two k's so that the lanes' halves read LDS banks 32 apart:
//     instruction i of a row product contracts dims dim_of(i, 0) and dim_of(i, 1) = that + 32.
//   * ONE 64-register prefetch buffer that the two streamed tiles take turns in, instead of one buffer per tile: the global
//     loads of a tile are issued when its LDS tile has been read for the last time and land while the other tile is
//     multiplied (64 MFMAs, ~4000 cycles).  The dK / dV kernel holds 128 registers of K and V and 128 of accumulators: there
//     the next dO tile is fetched only when a tile step is over, the one load left uncovered, which is what keeps the
//     kernel inside the register file without scratch.
//
// Why not two waves per 64-dim half with the partial S / dP added through LDS: it halves the registers of a wave but puts
// two workgroup barriers and an LDS round trip of S and dP into every tile step, and makes the zero-tile shortcut a decision
// two waves have to agree on; a wave that owns whole rows needs neither, and the register file holds it.
#include <algorithm>
#include <cmath>

#include "attention_common.h"

namespace pk2 {
namespace a128 {

constexpr int kD = 128;            // head size served
constexpr int kLd = 129;           // LDS row pitch of a staged 32 x 128 tile: rows on different banks
constexpr int kTileFloats = kAT * kLd;
constexpr int kNR = kD / 2;        // registers of a row operand = MFMA instructions of a row product
constexpr int kNB = kD / 32;       // 32-dim blocks of a transposed accumulator

// One staged tile on its way from global memory to LDS: rows [r0, r0 + 32), 128 columns; an instruction covers 2 whole rows.
struct TileRegs { float4 v[16]; };
__device__ __forceinline__ void fetch_tile(const float* __restrict__ base, int64_t rs, int r0, int T, TileRegs& t) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int row = it * 2 + (lane >> 5), col = (lane & 31) * 4;
    // No branch per row: a row behind the sequence reads the last row (r0 < T always) and is cleared with a bit mask -- a
    // select between the loaded value and zero is turned back into a branch around the load, 16 of them per tile.
    const float4 v = *reinterpret_cast<const float4*>(base + (int64_t)min(r0 + row, T - 1) * rs + col);
    const uint32_t keep = r0 + row < T ? 0xFFFFFFFFu : 0u;
    t.v[it] = make_float4(__uint_as_float(__float_as_uint(v.x) & keep), __uint_as_float(__float_as_uint(v.y) & keep),
                          __uint_as_float(__float_as_uint(v.z) & keep), __uint_as_float(__float_as_uint(v.w) & keep));
  }
}
__device__ __forceinline__ void put_tile(const TileRegs& t, float* tile) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    float* o = tile + (it * 2 + (lane >> 5)) * kLd + (lane & 31) * 4;
    o[0] = t.v[it].x; o[1] = t.v[it].y; o[2] = t.v[it].z; o[3] = t.v[it].w;
  }
}
__device__ __forceinline__ void scale_tile(TileRegs& t, float s) {
#pragma unroll
  for (int it = 0; it < 16; ++it) t.v[it] = make_float4(t.v[it].x * s, t.v[it].y * s, t.v[it].z * s, t.v[it].w * s);
}
// Every element of the tile is (+-) zero (attention.hip: tile_is_zero).
__device__ __forceinline__ bool tile_is_zero(const TileRegs& t) {
  unsigned any = 0u;
#pragma unroll
  for (int it = 0; it < 16; ++it)
    any |= (__float_as_uint(t.v[it].x) | __float_as_uint(t.v[it].y) | __float_as_uint(t.v[it].z) | __float_as_uint(t.v[it].w)) << 1;
  return __ballot(any != 0u) == 0ull;
}
// dim the MFMA instruction i of a row product contracts in the lanes' half hi, relative to 32 hi
__device__ __forceinline__ int dim_of(int i) { return (i & 31) + 64 * (i >> 5); }
// "row operand" of a staged tile: lane (row = lane % 32, hi = lane / 32) -> tile[row][32 hi + dim_of(i)], i < 64
__device__ __forceinline__ void load_rows(const float* tile, float (&r)[kNR]) {
  const int lane = threadIdx.x & 63;
  const float* src = tile + (lane & 31) * kLd + 32 * (lane >> 5);
#pragma unroll
  for (int i = 0; i < kNR; ++i) r[i] = src[dim_of(i)];
}
// acc[dim][n] += sum_rows tile[row][dim] * w[row][n] for the 128 dims (four 32-row blocks of the output), the weights w being
// an accumulator-layout register set (register j <-> tile rows row_of(j, hi)).
__device__ __forceinline__ void mfma_tile_t(const float* tile, const f32x16& w, f32x16 (&acc)[kNB]) {
  const int lane = threadIdx.x & 63, hi = lane >> 5, m = lane & 31;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float* src = tile + row_of(j, hi) * kLd + m;
#pragma unroll
    for (int c = 0; c < kNB; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[32 * c], w[j], acc[c], 0, 0, 0);
  }
}
// acc[row][n] = sum_dim tile[row][dim] * b[dim][n], b = a "row operand" register set of the n side
__device__ __forceinline__ f32x16 mfma_rows(const float* tile, const float (&b)[kNR]) {
  const int lane = threadIdx.x & 63;
  const float* src = tile + (lane & 31) * kLd + 32 * (lane >> 5);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int i = 0; i < kNR; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(src[dim_of(i)], b[i], acc, 0, 0, 0);
  return acc;
}
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[kNB]) {
#pragma unroll
  for (int c = 0; c < kNB; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
}
// The 128 floats of query/key row `row`, of which a lane holds dims 32 c + 8 g + 4 hi + (0..3) in the transposed
// accumulators -> out[row][...] (16 float4 stores), scaled.
__device__ __forceinline__ void store_t(float* out_row, int hi, const f32x16 (&acc)[kNB], float s) {
#pragma unroll
  for (int c = 0; c < kNB; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(out_row + 32 * c + 8 * g + 4 * hi) =
          make_float4(acc[c][4 * g] * s, acc[c][4 * g + 1] * s, acc[c][4 * g + 2] * s, acc[c][4 * g + 3] * s);
}
// The waves' accumulators summed by wave 0 through LDS ([64 regs][64 lanes] per wave, over the waves' tiles).
__device__ __forceinline__ void spill_acc(float* red, int lane, const f32x16 (&acc)[kNB], float s) {
#pragma unroll
  for (int c = 0; c < kNB; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(c * 16 + r) * 64 + lane] = acc[c][r] * s;
}
__device__ __forceinline__ void sum_acc(const float (*lds)[2 * kTileFloats], int lane, f32x16 (&acc)[kNB]) {
#pragma unroll
  for (int c = 0; c < kNB; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < kAWaves; ++k) a += lds[k][(c * 16 + r) * 64 + lane];
      acc[c][r] = a;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * kAWaves) attn128_fwd_kernel(AttnParams p) {
  __shared__ __attribute__((aligned(16))) float lds[kAWaves][2 * kTileFloats];
  __shared__ float stat[kAWaves][2][kAT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 5, qi = lane & 31;
  const int z = blockIdx.y, b = z / p.H, h = z % p.H, q0 = blockIdx.x * kAT, T = p.T;
  const int C = p.H * kD;
  const int64_t rs = (int64_t)p.B * 3 * C;                      // floats between consecutive frames of one utterance
  const float* Q = p.qkv + (int64_t)b * 3 * C + h * kD;
  const float* K = Q + C;
  const float* V = Q + 2 * C;
  float* Ks = lds[w]; float* Vs = lds[w] + kTileFloats;
  float qreg[kNR];
  TileRegs tr;
  fetch_tile(Q, rs, q0, T, tr);
  put_tile(tr, Ks);
  wave_lds_sync();
  load_rows(Ks, qreg);
#pragma unroll
  for (int i = 0; i < kNR; ++i) qreg[i] *= p.scale;
  wave_lds_sync();
  float m = -INFINITY, l = 0.f;
  f32x16 o[kNB];
  zero_acc(o);
  const int q = q0 + qi;
  const int nkt = valid_key_tiles(p, b);
  if (w < nkt) fetch_tile(K, rs, w * kAT, T, tr);
  for (int kt = w; kt < nkt; kt += kAWaves) {
    const int k0 = kt * kAT;
    put_tile(tr, Ks);
    wave_lds_sync();
    fetch_tile(V, rs, k0, T, tr);                                // lands under the 64 MFMAs of S
    f32x16 s = mfma_rows(Ks, qreg);                              // S^T: register r <-> key k0 + row_of(r, hi), this lane's query
    put_tile(tr, Vs);
    wave_lds_sync();
    if (kt + kAWaves < nkt) fetch_tile(K, rs, k0 + kAWaves * kAT, T, tr);      // lands under the softmax and the 64 MFMAs of O
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] += mask_of(p, b, q, k0 + row_of(r, hi));
      mt = fmaxf(mt, s[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);
    if (__ballot(mn > -INFINITY) != 0ull) {                       // (a tile masked out for every query adds nothing)
      const float corr = (m == -INFINITY) ? 0.f : __expf(m - mn);
      float ls = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = (mn == -INFINITY) ? 0.f : __expf(s[r] - mn);
        ls += s[r];
      }
      ls += __shfl_xor(ls, 32, 64);
      l = l * corr + ls;
      m = mn;
#pragma unroll
      for (int c = 0; c < kNB; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[c][r] *= corr;
      if (p.dropout) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= attn_keep(p, ((int64_t)z * T + q) * T + k0 + row_of(r, hi));
      }
      mfma_tile_t(Vs, s, o);
    }
    wave_lds_sync();
  }
  // merge the waves' partial results: the query of a lane is the same in every wave
  if (hi == 0) { stat[w][0][qi] = m; stat[w][1][qi] = l; }
  __syncthreads();
  float mstar = -INFINITY;
#pragma unroll
  for (int k = 0; k < kAWaves; ++k) mstar = fmaxf(mstar, stat[k][0][qi]);
  float lstar = 0.f;
#pragma unroll
  for (int k = 0; k < kAWaves; ++k) lstar += stat[k][0][qi] == -INFINITY ? 0.f : stat[k][1][qi] * __expf(stat[k][0][qi] - mstar);
  const float mine = (m == -INFINITY) ? 0.f : __expf(m - mstar);
  spill_acc(lds[w], lane, o, mine);
  __syncthreads();
  if (w == 0) {
    sum_acc(lds, lane, o);
    if (q < T) {
      const float inv = lstar > 0.f ? 1.0f / lstar : 0.f;
      store_t(p.ctx_out + ((int64_t)q * p.B + b) * C + h * kD, hi, o, inv);
      if (hi == 0) p.lse_out[(int64_t)z * T + q] = lstar > 0.f ? mstar + __logf(lstar) : -INFINITY;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward 1: dQ (and D = rowsum(dO * O)), owner = query tile, the key tiles dealt to the waves
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * kAWaves) attn128_bwd_dq_kernel(AttnParams p) {
  __shared__ __attribute__((aligned(16))) float lds[kAWaves][2 * kTileFloats];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 5, qi = lane & 31;
  const int z = blockIdx.y, b = z / p.H, h = z % p.H, q0 = blockIdx.x * kAT, T = p.T;
  const int C = p.H * kD;
  const int64_t rs = (int64_t)p.B * 3 * C, rc = (int64_t)p.B * C;
  const float* Q = p.qkv + (int64_t)b * 3 * C + h * kD;
  const float* K = Q + C;
  const float* V = Q + 2 * C;
  const float* O = p.ctx + (int64_t)b * C + h * kD;
  const float* dO = p.dctx + (int64_t)b * C + h * kD;
  float* Ks = lds[w]; float* Vs = lds[w] + kTileFloats;
  const int q = q0 + qi;
  float doreg[kNR];
  TileRegs tr;
  fetch_tile(dO, rc, q0, T, tr);
  const bool dz = (p.skip_pad & 2) && tile_is_zero(tr);         // dO of this query tile is all zero (every wave holds the same tile): D = 0, dQ = 0
  if (dz) {
    if (w == 0 && q < T) {
      if (hi == 0) p.dsum[(int64_t)z * T + q] = 0.f;
      f32x16 zero[kNB];
      zero_acc(zero);
      store_t(p.dqkv + ((int64_t)q * p.B + b) * 3 * C + h * kD, hi, zero, 1.0f);
    }
    return;
  }
  put_tile(tr, Vs);
  fetch_tile(O, rc, q0, T, tr);
  put_tile(tr, Ks);
  wave_lds_sync();
  load_rows(Vs, doreg);
  float dsum = 0.f;
  {
    const float* src = Ks + (lane & 31) * kLd + 32 * (lane >> 5);
#pragma unroll
    for (int i = 0; i < kNR; ++i) dsum += src[dim_of(i)] * doreg[i];
    dsum += __shfl_xor(dsum, 32, 64);
  }
  wave_lds_sync();
  float qreg[kNR];
  fetch_tile(Q, rs, q0, T, tr);
  put_tile(tr, Ks);
  wave_lds_sync();
  load_rows(Ks, qreg);
#pragma unroll
  for (int i = 0; i < kNR; ++i) qreg[i] *= p.scale;
  wave_lds_sync();
  const float lse = q < T ? p.lse_in[(int64_t)z * T + q] : -INFINITY;
  if (w == 0 && hi == 0 && q < T) p.dsum[(int64_t)z * T + q] = dsum;
  f32x16 g[kNB];
  zero_acc(g);
  const int nkt = valid_key_tiles(p, b);
  if (w < nkt) fetch_tile(K, rs, w * kAT, T, tr);
  for (int kt = w; kt < nkt; kt += kAWaves) {
    const int k0 = kt * kAT;
    put_tile(tr, Ks);
    wave_lds_sync();
    fetch_tile(V, rs, k0, T, tr);                                // lands under the 64 MFMAs of S
    f32x16 s = mfma_rows(Ks, qreg);
    put_tile(tr, Vs);
    wave_lds_sync();
    if (kt + kAWaves < nkt) fetch_tile(K, rs, k0 + kAWaves * kAT, T, tr);      // lands under dP and dQ
    f32x16 dp = mfma_rows(Vs, doreg);                            // dP^T[key][query] = V dO^T
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + row_of(r, hi);
      const float sv = s[r] + mask_of(p, b, q, k);
      const float pr = (lse == -INFINITY || sv == -INFINITY) ? 0.f : __expf(sv - lse);
      float d = dp[r];
      if (p.dropout) d *= attn_keep(p, ((int64_t)z * T + q) * T + k);
      s[r] = pr * (d - dsum) * p.scale;                          // dS^T
    }
    mfma_tile_t(Ks, s, g);                                       // dQ^T[dim][query] += K^T dS^T
    wave_lds_sync();
  }
  spill_acc(lds[w], lane, g, 1.0f);
  __syncthreads();
  if (w == 0) {
    sum_acc(lds, lane, g);
    if (q < T) store_t(p.dqkv + ((int64_t)q * p.B + b) * 3 * C + h * kD, hi, g, 1.0f);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward 2: dK, dV, owner = key tile, the query tiles dealt to the waves
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * kAWaves) attn128_bwd_dkv_kernel(AttnParams p) {
  __shared__ __attribute__((aligned(16))) float lds[kAWaves][2 * kTileFloats];
  __shared__ float qstat[kAWaves][2][kAT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 5, ki = lane & 31;
  const int z = blockIdx.y, b = z / p.H, h = z % p.H, k0 = blockIdx.x * kAT, T = p.T;
  const int C = p.H * kD;
  const int64_t rs = (int64_t)p.B * 3 * C, rc = (int64_t)p.B * C;
  const float* Q = p.qkv + (int64_t)b * 3 * C + h * kD;
  const float* K = Q + C;
  const float* V = Q + 2 * C;
  const float* dO = p.dctx + (int64_t)b * C + h * kD;
  float* Qs = lds[w]; float* Ds = lds[w] + kTileFloats;
  float kreg[kNR], vreg[kNR];
  TileRegs tr;
  fetch_tile(K, rs, k0, T, tr);
  put_tile(tr, Qs);
  fetch_tile(V, rs, k0, T, tr);
  put_tile(tr, Ds);
  wave_lds_sync();
  load_rows(Qs, kreg);
  load_rows(Ds, vreg);
  wave_lds_sync();
  const int k = k0 + ki;
  f32x16 gk[kNB], gv[kNB];
  zero_acc(gk);
  zero_acc(gv);
  // (the key of a lane is the same for every query tile: its padding is looked up once, and the 16 mask look-ups of a tile
  // are clamped loads instead of mask_of's branches -- with those in the loop the kernel needs 108 registers more)
  const bool kvalid = k < T && !(p.key_pad && p.key_pad[(int64_t)b * T + min(k, T - 1)]);
  const int nqt = blockIdx.x < valid_key_tiles(p, b) ? (T + kAT - 1) / kAT : 0;      // (a tile of padded keys: dK = dV = 0, stored below)
  if (w < nqt) fetch_tile(dO, rc, w * kAT, T, tr);
  for (int qt = w; qt < nqt; qt += kAWaves) {
    const int q0 = qt * kAT;
    const bool more = qt + kAWaves < nqt;
    if ((p.skip_pad & 2) && tile_is_zero(tr)) {                  // dO = 0 (and with it D = 0): dV += 0, dS = 0
      if (more) fetch_tile(dO, rc, q0 + kAWaves * kAT, T, tr);
      continue;
    }
    put_tile(tr, Ds);
    if (lane < kAT) {
      const int q = q0 + lane;
      qstat[w][0][lane] = q < T ? p.lse_in[(int64_t)z * T + q] : -INFINITY;
      qstat[w][1][lane] = q < T ? p.dsum[(int64_t)z * T + q] : 0.f;
    }
    wave_lds_sync();
    fetch_tile(Q, rs, q0, T, tr);                                // lands under the 64 MFMAs of dP
    f32x16 dp = mfma_rows(Ds, vreg);                             // dP[query][key] = dO V^T
    // Q is staged pre-scaled, as the forward and dQ kernels hold it: the products and their order are then the forward's, S
    // is the forward's bit for bit, and exp(S - lse) sums to 1 over a row as it did there.  128 ** -0.5 is no power of two:
    // scaling the sum instead rounds S another way, and where a few keys carry a row (|S| ~ 30) the 1e-5 between the two
    // roundings is a relative 1e-5 on every P, which nothing normalises here.
    scale_tile(tr, p.scale);
    put_tile(tr, Qs);
    wave_lds_sync();
    f32x16 s = mfma_rows(Qs, kreg);                              // S[query][key]: register r <-> query q0 + row_of(r, hi), this lane's key
    f32x16 pd;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = q0 + row_of(r, hi);
      const float lse = qstat[w][0][row_of(r, hi)], dsum = qstat[w][1][row_of(r, hi)];
      float sv = s[r];
      if (p.src_mask) sv += p.src_mask[(int64_t)min(q, T - 1) * T + min(k, T - 1)];
      const float pr = (!kvalid || q >= T || lse == -INFINITY || sv == -INFINITY) ? 0.f : __expf(sv - lse);
      const float keep = p.dropout ? attn_keep(p, ((int64_t)z * T + q) * T + k) : 1.0f;
      pd[r] = pr * keep;                                         // dropped-out probabilities: dV = P_d^T dO
      s[r] = pr * (dp[r] * keep - dsum);                         // dS (its factor `scale` is in the staged Q)
    }
    mfma_tile_t(Ds, pd, gv);                                     // dV^T[dim][key] += dO^T P_d
    mfma_tile_t(Qs, s, gk);                                      // dK^T[dim][key] += (scale Q)^T dS
    wave_lds_sync();
    // (the one load of this file that nothing covers: issued any earlier, the 64 registers it lands in are live through the
    // two transposed products next to K, V, dK, dV, dS and P_d, and the kernel spills 108 of them)
    if (more) fetch_tile(dO, rc, q0 + kAWaves * kAT, T, tr);
  }
  auto reduce_store = [&](f32x16 (&a)[kNB], int part) {
    spill_acc(lds[w], lane, a, 1.0f);
    __syncthreads();
    if (w == 0) {
      sum_acc(lds, lane, a);
      if (k < T) store_t(p.dqkv + ((int64_t)k * p.B + b) * 3 * C + part * C + h * kD, hi, a, 1.0f);
    }
    __syncthreads();
  };
  reduce_store(gk, 1);
  reduce_store(gv, 2);
}

}  // namespace a128

void attn128_launch_fwd(const AttnParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(a128::attn128_fwd_kernel, dim3((p.T + kAT - 1) / kAT, p.B * p.H), dim3(64 * kAWaves), 0, stream, p);
}

void attn128_launch_bwd(const AttnParams& p, int parts, hipStream_t stream) {
  const dim3 grid((p.T + kAT - 1) / kAT, p.B * p.H), block(64 * kAWaves);
  if (parts & 1) hipLaunchKernelGGL(a128::attn128_bwd_dq_kernel, grid, block, 0, stream, p);
  if (parts & 2) hipLaunchKernelGGL(a128::attn128_bwd_dkv_kernel, grid, block, 0, stream, p);
}

}  // namespace pk2
