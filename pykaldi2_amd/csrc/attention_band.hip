// Fused multi-head self-attention over a context band for gfx950 (f32 MFMA, head sizes 64 and 128): the contract of
// attention.hip / attention128.hip (read the header of attention.hip first: packed qkv, transposed 32 x 32 tiles on
// v_mfma_f32_32x32x2_f32, P in the accumulator registers, in-lane row statistics, backward by recomputation from lse, the
// dropout mask of dropout.hip indexed as [B*H][T][T]) with the additive [T][T] mask replaced by three integers (left,
// right, chunk): query q sees the keys of an interval (attention_band.h), so the kernels know from the tile indices alone
// which (query tile, key tile) pairs hold anything, and multiply only those.
//
// A band is narrow: a query tile meets two or three key tiles, not T / 32.  Dealing those to four waves and merging their
// partial rows through LDS, as the dense kernels do, would leave most waves idle and the merge the larger part of the work.
// Here a WAVE owns a whole tile of rows and a workgroup four consecutive ones:
//
//   forward, dQ   wave w <- query tile 4 x + w; it walks the key tiles [lo_w, hi_w) its band reaches, clipped to the
//                 utterance's valid key tiles.  The four ranges are shifted copies of one another, so the workgroup walks
//                 their union once: all 256 threads stage each K tile and each V tile into LDS once, and every wave
//                 multiplies a staged pair only if it lies in its own range.  A wave holds complete rows: no merge, the
//                 results go from the accumulators to memory.
//   dK / dV       the mirror image: wave w <- key tile 4 x + w, the union of the four query-tile ranges is walked once with
//                 Q (pre-scaled, as the forward holds it), dO, lse and dsum staged for all four waves.  The query range of a
//                 key is the inverse of the interval (band_query_lo / _hi): with chunk > 1 its ends are chunk ends.
//
// The ring: kBRing = 2 staged pairs.  In step i the workgroup writes pair i + 1 from registers into the slot step i - 1
// read, issues the global loads of pair i + 2 into those registers, multiplies pair i, and meets at ONE barrier -- the
// registers are the third stage, so a deeper ring would hide nothing more and only cost the LDS that lets two workgroups
// share a CU at head size 64.  Staged by 256 threads a pair in flight is 16 (head size 64) or 32 (128) registers per thread,
// a quarter of what a wave staging its own tiles holds.
//
// Visibility is one 32-bit word per lane and tile: bit i <-> key (query) i of the tile.  Key padding and k < T arrive as a
// ballot with the staged tile; a lane's own interval is constant over the walk, so an edge tile costs two shifts
// (interval_bits) and a tile wholly inside the band of all 32 rows skips even that.  Early query tiles of a causal band
// (left = -1) walk fewer key tiles than late ones, so the workgroups of an utterance finish at different times: accepted,
// the grid is many times the CU count.  No atomics, nothing between workgroups: a call gives the same bits alone or in a batch.
#include <algorithm>
#include <climits>

#include "attention_band.h"

namespace pk2 {

struct TileRange { int lo, hi; };          // tiles [lo, hi); empty if lo >= hi

// key tiles, of an utterance's first n, that the queries [q0, q0 + 32) see
__device__ __forceinline__ TileRange key_tiles(const Band& bd, int q0, int T, int n) {
  if (q0 >= T) return TileRange{0, 0};
  return TileRange{band_key_lo(bd, q0) / kAT, min(n, band_key_hi(bd, min(q0 + kAT, T) - 1, T) / kAT + 1)};
}
// query tiles that see the keys [k0, k0 + 32); none for a tile behind the utterance's n valid key tiles
__device__ __forceinline__ TileRange query_tiles(const Band& bd, int k0, int T, int n) {
  if (k0 >= n * kAT) return TileRange{0, 0};
  return TileRange{band_query_lo(bd, k0) / kAT, band_query_hi(bd, min(k0 + kAT, T) - 1, T) / kAT + 1};
}
// what the workgroup walks: from the first tile of any of its waves' ranges to the last
template <class F>
__device__ __forceinline__ TileRange union_of_waves(F range_of_wave) {
  TileRange u{INT_MAX, 0};
#pragma unroll
  for (int w = 0; w < kAWaves; ++w) {
    const TileRange r = range_of_wave(w);
    if (r.lo < r.hi) { u.lo = min(u.lo, r.lo); u.hi = max(u.hi, r.hi); }
  }
  return u;
}
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// A tile pair (and the words that go with it) on its way from global memory to the ring.
template <int D>
struct Staged {
  typename BandTile<D>::template Regs<kBThreads> a, b;
  uint32_t word;
};

// ---------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kBThreads, D == 64 ? 2 : 1) attn_band_fwd_kernel(AttnParams p, Band bd) {
  using X = BandTile<D>;
  __shared__ __attribute__((aligned(16))) float ring[kBRing][2][X::kFloats];
  __shared__ uint32_t keybits[kBRing];                           // bit i: key i of the staged tile is inside T and not padded
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hi = lane >> 5, qi = lane & 31;
  const int z = blockIdx.y, b = z / p.H, h = z % p.H, T = p.T, C = p.H * D;
  const int qt0 = blockIdx.x * kAWaves, q0 = (qt0 + w) * kAT, q = q0 + qi;
  const int64_t rs = (int64_t)p.B * 3 * C;                      // floats between consecutive frames of one utterance
  const float* Q = p.qkv + (int64_t)b * 3 * C + h * D;
  const float* K = Q + C;
  const float* V = Q + 2 * C;
  const uint8_t* kp = p.key_pad ? p.key_pad + (int64_t)b * T : nullptr;
  float qreg[X::kNR];
  X::load_rows(Q, rs, q0, T, &ring[0][0][0] + w * X::kFloats, p.scale, qreg);
  const int nkt = valid_key_tiles(p, b);
  TileRange mine = key_tiles(bd, q0, T, nkt);
  mine.lo = uniform(mine.lo); mine.hi = uniform(mine.hi);
  const TileRange all = union_of_waves([&](int ww) { return key_tiles(bd, (qt0 + ww) * kAT, T, nkt); });
  const int n = all.lo < all.hi ? all.hi - all.lo : 0;
  // a key tile from inside_lo on and up to inside_hi is seen whole by all 32 queries; this lane's query sees [klo, khi]
  const int qlast = min(q0 + kAT, T) - 1;
  const int inside_lo = uniform(band_key_lo(bd, max(qlast, 0))), inside_hi = uniform(band_key_hi(bd, min(q0, T - 1), T));
  const int klo = band_key_lo(bd, min(q, T - 1)), khi = band_key_hi(bd, min(q, T - 1), T);
  Staged<D> st;
  st.word = 0u;
  auto fetch = [&](int kt) {
    X::template fetch<kBThreads>(K, rs, kt * kAT, T, tid, st.a);
    X::template fetch<kBThreads>(V, rs, kt * kAT, T, tid, st.b);
    const int k = kt * kAT + tid;
    st.word = tid < kAT && k < T && !(kp && kp[k]);
  };
  auto put = [&](int slot) {
    X::template put<kBThreads>(st.a, ring[slot][0], tid);
    X::template put<kBThreads>(st.b, ring[slot][1], tid);
    const uint64_t bits = __ballot(st.word != 0u);
    if (tid == 0) keybits[slot] = (uint32_t)bits;
  };
  float m = -INFINITY, l = 0.f;
  f32x16 o[X::kNB];
  X::zero_acc(o);
  __syncthreads();                                               // (the waves' own tiles above are the ring's)
  if (n > 0) { fetch(all.lo); put(0); }
  if (n > 1) fetch(all.lo + 1);
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const int kt = all.lo + i, k0 = kt * kAT, slot = i % kBRing;
    if (i + 1 < n) put((i + 1) % kBRing);
    if (i + 2 < n) fetch(kt + 2);
    if (kt >= mine.lo && kt < mine.hi) {
      const float* Ks = ring[slot][0];
      const float* Vs = ring[slot][1];
      uint32_t vis = keybits[slot];
      if (k0 < inside_lo || k0 + kAT - 1 > inside_hi) vis &= interval_bits(klo, khi, k0);      // an edge tile
      f32x16 s = X::mfma_rows(Ks, qreg);                         // S^T: register r <-> key k0 + row_of(r, hi), this lane's query
      float mt = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = (vis >> row_of(r, hi)) & 1u ? s[r] : -INFINITY;
        mt = fmaxf(mt, s[r]);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float mn = fmaxf(m, mt);
      if (__ballot(mn > -INFINITY) != 0ull) {                     // (a tile no query of the wave sees anything of adds nothing)
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
        for (int c = 0; c < X::kNB; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[c][r] *= corr;
        if (p.dropout) {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] *= attn_keep(p, ((int64_t)z * T + q) * T + k0 + row_of(r, hi));
        }
        X::mfma_tile_t(Vs, s, o);
      }
    }
    __syncthreads();
  }
  if (q < T) {
    X::store_t(p.ctx_out + ((int64_t)q * p.B + b) * C + h * D, hi, o, l > 0.f ? 1.0f / l : 0.f);
    if (hi == 0) p.lse_out[(int64_t)z * T + q] = l > 0.f ? m + __logf(l) : -INFINITY;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward 1: dQ (and D = rowsum(dO * O)), the forward's walk
// ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kBThreads, D == 64 ? 2 : 1) attn_band_dq_kernel(AttnParams p, Band bd) {
  using X = BandTile<D>;
  __shared__ __attribute__((aligned(16))) float ring[kBRing][2][X::kFloats];
  __shared__ uint32_t keybits[kBRing];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hi = lane >> 5, qi = lane & 31;
  const int z = blockIdx.y, b = z / p.H, h = z % p.H, T = p.T, C = p.H * D;
  const int qt0 = blockIdx.x * kAWaves, q0 = (qt0 + w) * kAT, q = q0 + qi;
  const int64_t rs = (int64_t)p.B * 3 * C, rc = (int64_t)p.B * C;
  const float* Q = p.qkv + (int64_t)b * 3 * C + h * D;
  const float* K = Q + C;
  const float* V = Q + 2 * C;
  const float* O = p.ctx + (int64_t)b * C + h * D;
  const float* dO = p.dctx + (int64_t)b * C + h * D;
  const uint8_t* kp = p.key_pad ? p.key_pad + (int64_t)b * T : nullptr;
  float* own = &ring[0][0][0] + w * X::kFloats;
  float qreg[X::kNR], doreg[X::kNR];
  X::load_rows(dO, rc, q0, T, own, 1.0f, doreg);
  // D = rowsum(dO * O) as the diagonal of the MFMA product O dO^T: the sum of a row then runs in the order dP = V dO^T is
  // summed in below, and for a query that sees ONE key (P = 1, O = V: a band's first rows, the diagonal band) dP - D is
  // exactly 0, as it is in exact arithmetic, instead of the difference of two roundings of the same sum.
  float dsum = 0.f;
  {
    typename X::template Regs<64> x;
    X::template fetch<64>(O, rc, q0, T, lane, x);
    X::template put<64>(x, own, lane);
    wave_lds_sync();
    const f32x16 od = X::mfma_rows(own, doreg);                  // register r <-> row row_of(r, hi) of O, this lane's query
#pragma unroll
    for (int r = 0; r < 16; ++r) dsum = row_of(r, hi) == qi ? od[r] : dsum;
    dsum += __shfl_xor(dsum, 32, 64);                            // (the lanes' other half holds no row of this query: + 0)
    wave_lds_sync();
  }
  X::load_rows(Q, rs, q0, T, own, p.scale, qreg);
  const float lse = q < T ? p.lse_in[(int64_t)z * T + q] : -INFINITY;
  if (hi == 0 && q < T) p.dsum[(int64_t)z * T + q] = dsum;
  const int nkt = valid_key_tiles(p, b);
  TileRange mine = key_tiles(bd, q0, T, nkt);
  mine.lo = uniform(mine.lo); mine.hi = uniform(mine.hi);
  const TileRange all = union_of_waves([&](int ww) { return key_tiles(bd, (qt0 + ww) * kAT, T, nkt); });
  const int n = all.lo < all.hi ? all.hi - all.lo : 0;
  const int qlast = min(q0 + kAT, T) - 1;
  const int inside_lo = uniform(band_key_lo(bd, max(qlast, 0))), inside_hi = uniform(band_key_hi(bd, min(q0, T - 1), T));
  const int klo = band_key_lo(bd, min(q, T - 1)), khi = band_key_hi(bd, min(q, T - 1), T);
  Staged<D> st;
  st.word = 0u;
  auto fetch = [&](int kt) {
    X::template fetch<kBThreads>(K, rs, kt * kAT, T, tid, st.a);
    X::template fetch<kBThreads>(V, rs, kt * kAT, T, tid, st.b);
    const int k = kt * kAT + tid;
    st.word = tid < kAT && k < T && !(kp && kp[k]);
  };
  auto put = [&](int slot) {
    X::template put<kBThreads>(st.a, ring[slot][0], tid);
    X::template put<kBThreads>(st.b, ring[slot][1], tid);
    const uint64_t bits = __ballot(st.word != 0u);
    if (tid == 0) keybits[slot] = (uint32_t)bits;
  };
  f32x16 g[X::kNB];
  X::zero_acc(g);
  __syncthreads();
  if (n > 0) { fetch(all.lo); put(0); }
  if (n > 1) fetch(all.lo + 1);
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const int kt = all.lo + i, k0 = kt * kAT, slot = i % kBRing;
    if (i + 1 < n) put((i + 1) % kBRing);
    if (i + 2 < n) fetch(kt + 2);
    if (kt >= mine.lo && kt < mine.hi) {
      const float* Ks = ring[slot][0];
      const float* Vs = ring[slot][1];
      uint32_t vis = keybits[slot];
      if (k0 < inside_lo || k0 + kAT - 1 > inside_hi) vis &= interval_bits(klo, khi, k0);
      f32x16 s = X::mfma_rows(Ks, qreg);
      f32x16 dp = X::mfma_rows(Vs, doreg);                       // dP^T[key][query] = V dO^T
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool seen = (vis >> row_of(r, hi)) & 1u;
        const float pr = (lse == -INFINITY || !seen) ? 0.f : __expf(s[r] - lse);
        float d = dp[r];
        if (p.dropout) d *= attn_keep(p, ((int64_t)z * T + q) * T + k0 + row_of(r, hi));
        s[r] = pr * (d - dsum) * p.scale;                        // dS^T
      }
      X::mfma_tile_t(Ks, s, g);                                  // dQ^T[dim][query] += K^T dS^T
    }
    __syncthreads();
  }
  if (q < T) X::store_t(p.dqkv + ((int64_t)q * p.B + b) * 3 * C + h * D, hi, g, 1.0f);
}

// ---------------------------------------------------------------------------------------------------------------
// backward 2: dK, dV, owner = key tile, the walk over the query tiles that see it
// ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kBThreads) attn_band_dkv_kernel(AttnParams p, Band bd) {
  using X = BandTile<D>;
  __shared__ __attribute__((aligned(16))) float ring[kBRing][2][X::kFloats];
  __shared__ float qstat[kBRing][2][kAT];                        // lse and dsum of the staged tile's queries
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hi = lane >> 5, ki = lane & 31;
  const int z = blockIdx.y, b = z / p.H, h = z % p.H, T = p.T, C = p.H * D;
  const int kt0 = blockIdx.x * kAWaves, k0 = (kt0 + w) * kAT, k = k0 + ki;
  const int64_t rs = (int64_t)p.B * 3 * C, rc = (int64_t)p.B * C;
  const float* Q = p.qkv + (int64_t)b * 3 * C + h * D;
  const float* K = Q + C;
  const float* V = Q + 2 * C;
  const float* dO = p.dctx + (int64_t)b * C + h * D;
  float* tile = &ring[0][0][0] + w * X::kFloats;
  float kreg[X::kNR], vreg[X::kNR];
  X::load_rows(K, rs, k0, T, tile, 1.0f, kreg);
  X::load_rows(V, rs, k0, T, tile, 1.0f, vreg);
  const bool kvalid = k < T && !(p.key_pad && p.key_pad[(int64_t)b * T + min(k, T - 1)]);
  const int nkt = valid_key_tiles(p, b);                         // (a tile of padded keys walks nothing: dK = dV = 0, stored below)
  TileRange mine = query_tiles(bd, k0, T, nkt);
  mine.lo = uniform(mine.lo); mine.hi = uniform(mine.hi);
  const TileRange all = union_of_waves([&](int ww) { return query_tiles(bd, (kt0 + ww) * kAT, T, nkt); });
  const int n = all.lo < all.hi ? all.hi - all.lo : 0;
  // a query tile from inside_lo on and up to inside_hi sees all 32 keys whole; this lane's key is seen by [qlo, qhi]
  const int klast = min(k0 + kAT, T) - 1;
  const int inside_lo = uniform(band_query_lo(bd, max(klast, 0))), inside_hi = uniform(band_query_hi(bd, min(k0, T - 1), T));
  const int qlo = band_query_lo(bd, min(k, T - 1)), qhi = band_query_hi(bd, min(k, T - 1), T);
  Staged<D> st;
  st.word = 0u;
  auto fetch = [&](int qt) {
    X::template fetch<kBThreads>(Q, rs, qt * kAT, T, tid, st.a);
    X::template fetch<kBThreads>(dO, rc, qt * kAT, T, tid, st.b);
    if (tid < 2 * kAT) {
      const int q = qt * kAT + (tid & 31);
      const float* src = tid < kAT ? p.lse_in : p.dsum;
      st.word = __float_as_uint(q < T ? src[(int64_t)z * T + q] : (tid < kAT ? -INFINITY : 0.f));
    }
  };
  auto put = [&](int slot) {
    // Q is staged pre-scaled, as the forward and dQ kernels hold it: S is then the forward's bit for bit and exp(S - lse)
    // sums to 1 over a row as it did there (attention128.hip); the factor `scale` of dS is in it as well.
    X::template put<kBThreads>(st.a, ring[slot][0], tid, p.scale);
    X::template put<kBThreads>(st.b, ring[slot][1], tid);
    if (tid < 2 * kAT) qstat[slot][tid >> 5][tid & 31] = __uint_as_float(st.word);
  };
  f32x16 gk[X::kNB], gv[X::kNB];
  X::zero_acc(gk);
  X::zero_acc(gv);
  __syncthreads();
  if (n > 0) { fetch(all.lo); put(0); }
  if (n > 1) fetch(all.lo + 1);
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const int qt = all.lo + i, q0 = qt * kAT, slot = i % kBRing;
    if (i + 1 < n) put((i + 1) % kBRing);
    // Head size 128 holds 256 registers of K, V, dK and dV: the pair in flight joins them only when P_d is spent, under the
    // 64 MFMAs of dK (issued before the products, the kernel spills)
    const bool more = i + 2 < n, own = qt >= mine.lo && qt < mine.hi, late = D == 128 && own;
    if (more && !late) fetch(qt + 2);
    if (own) {
      const float* Qs = ring[slot][0];
      const float* Ds = ring[slot][1];
      uint32_t vis = kvalid ? 0xFFFFFFFFu : 0u;
      if (q0 < inside_lo || q0 + kAT - 1 > inside_hi) vis &= interval_bits(qlo, qhi, q0);
      f32x16 s = X::mfma_rows(Qs, kreg);                         // S[query][key]: register r <-> query q0 + row_of(r, hi), this lane's key
      f32x16 dp = X::mfma_rows(Ds, vreg);                        // dP[query][key] = dO V^T
      f32x16 pd;                                                 // dropped-out probabilities: dV = P_d^T dO
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row_of(r, hi);
        const float lse = qstat[slot][0][row];
        s[r] = (!((vis >> row) & 1u) || lse == -INFINITY) ? 0.f : __expf(s[r] - lse);      // P
        pd[r] = s[r];
      }
      if (p.dropout) {                                           // (one branch around all 16 draws: one per draw costs 50 registers)
        const int64_t at = ((int64_t)z * T + q0 + 4 * hi) * T + k;      // the dropout matrix at (the lanes' first query, key)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float keep = attn_keep(p, at + (int64_t)row_of(r, 0) * T);
          pd[r] *= keep;
          dp[r] *= keep;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] *= dp[r] - qstat[slot][1][row_of(r, hi)];      // dS (its factor `scale` is in the staged Q)
      X::mfma_tile_t(Ds, pd, gv);                                // dV^T[dim][key] += dO^T P_d
      if (late) {                                                // (cleared where nothing follows: live through the products otherwise)
        if (more) fetch(qt + 2); else st = Staged<D>{};
      }
      X::mfma_tile_t(Qs, s, gk);                                 // dK^T[dim][key] += (scale Q)^T dS
    }
    __syncthreads();
  }
  if (k < T) {
    float* out = p.dqkv + ((int64_t)k * p.B + b) * 3 * C + h * D;
    X::store_t(out + C, hi, gk, 1.0f);
    X::store_t(out + 2 * C, hi, gv, 1.0f);
  }
}

template <int D>
static void launch_band(const AttnParams& p, const Band& bd, int parts, hipStream_t stream) {      // parts: bit 0 forward, 1 dQ, 2 dK / dV
  const int tiles = (p.T + kAT - 1) / kAT;
  const dim3 grid((tiles + kAWaves - 1) / kAWaves, p.B * p.H), block(kBThreads);
  if (parts & 1) hipLaunchKernelGGL(attn_band_fwd_kernel<D>, grid, block, 0, stream, p, bd);
  if (parts & 2) hipLaunchKernelGGL(attn_band_dq_kernel<D>, grid, block, 0, stream, p, bd);
  if (parts & 4) hipLaunchKernelGGL(attn_band_dkv_kernel<D>, grid, block, 0, stream, p, bd);
}

}  // namespace pk2

using namespace pk2;

static int band_fill(Band* bd, int32_t T, int32_t left, int32_t right, int32_t chunk) {
  PK2_REQUIRE(left >= -1 && right >= -1 && chunk >= 1,
              "attention_band: a band is left >= -1, right >= -1, chunk >= 1 (got %d, %d, %d)", left, right, chunk);
  // (more context than there are frames is all of them: the same intervals, and no sum of two of these leaves int32)
  bd->left = std::min(left, T); bd->right = std::min(right, T); bd->chunk = std::min(chunk, T);
  return PK2_OK;
}

extern "C" int pk2_attention_band_fwd(const float* qkv, int32_t T, int32_t B, int32_t H, int32_t head_dim, float scale,
                                      int32_t left, int32_t right, int32_t chunk, const uint8_t* key_padding, float dropout_p,
                                      uint64_t seed, float* ctx, float* lse, void* stream_) {
  PK2_REQUIRE(qkv && ctx && lse, "attention_band_fwd: null pointer");
  AttnParams p{};
  Band bd{};
  int rc = attn_fill(&p, T, B, H, head_dim, scale, nullptr, key_padding, dropout_p, seed);
  if (!rc) rc = band_fill(&bd, T, left, right, chunk);
  if (rc) return rc;
  p.qkv = qkv; p.ctx_out = ctx; p.lse_out = lse;
  if (head_dim == 64) launch_band<64>(p, bd, 1, static_cast<hipStream_t>(stream_));
  else launch_band<128>(p, bd, 1, static_cast<hipStream_t>(stream_));
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_attention_band_bwd(const float* qkv, const float* ctx, const float* dctx, const float* lse, int32_t T,
                                      int32_t B, int32_t H, int32_t head_dim, float scale, int32_t left, int32_t right,
                                      int32_t chunk, const uint8_t* key_padding, float dropout_p, uint64_t seed, float* dqkv,
                                      float* dsum, void* stream_) {
  PK2_REQUIRE(qkv && ctx && dctx && lse && dqkv && dsum, "attention_band_bwd: null pointer");
  AttnParams p{};
  Band bd{};
  int rc = attn_fill(&p, T, B, H, head_dim, scale, nullptr, key_padding, dropout_p, seed);
  if (!rc) rc = band_fill(&bd, T, left, right, chunk);
  if (rc) return rc;
  p.qkv = qkv; p.ctx = ctx; p.dctx = dctx; p.lse_in = lse; p.dqkv = dqkv; p.dsum = dsum;
  if (head_dim == 64) launch_band<64>(p, bd, 6, static_cast<hipStream_t>(stream_));
  else launch_band<128>(p, bd, 6, static_cast<hipStream_t>(stream_));
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
