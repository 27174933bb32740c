// What the beam searches share on the device (ctc_beam.hip, transducer_beam.hip): the 64-bit keys, the
// prefix hash, the select of the `want` largest candidates and the tail that turns the final beam into the outputs.  Both
// searches run one workgroup of kBeamThreads threads per utterance; the beam layouts, the per-frame logic and the row passes
// are their own.  beam_select is ctcb_search's today: tb_search keeps its one-candidate tb_select, which measured faster
// there (profiles/beam_shared_ab.txt), and shares the rest.
#pragma once
#include "common.h"

namespace pk2 {

typedef unsigned long long u64;

constexpr int kBeamThreads = 1024;
constexpr int kBeamWaves = kBeamThreads / 64;

__device__ __forceinline__ u64 wave_max64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const u64 w = shfl_xor64(v, o); v = w > v ? w : v; }
  return v;
}

// (logit, column) as one key: a larger logit is a larger key, and of equal logits the lower column
__device__ __forceinline__ u64 beam_key(float v, int col) {
  const unsigned b = __float_as_uint(v), u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((u64)u << 32) | (0xFFFFFFFFu - (unsigned)col);
}
__device__ __forceinline__ int beam_key_col(u64 key) { return (int)(0xFFFFFFFFu - (unsigned)key); }
// a double's bits in the order of the doubles (never 0 for a double that is not NaN)
__device__ __forceinline__ u64 beam_ordered(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

constexpr u64 kHashEmpty = 0x243F6A8885A308D3ull;
__device__ __forceinline__ u64 beam_mix(u64 h, int c) {      // the hash of prefix + c from the hash of the prefix (splitmix64's finish)
  u64 z = h ^ ((u64)(unsigned)(c + 1) * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The `want` largest keys of candidates 0 .. count - 1, survivors in candidate order.  A thread owns the cpt <= CPT consecutive
// candidates from `first` on, key[q] that of candidate first + q (and count <= kBeamThreads cpt); slot[q] is its slot among
// the survivors or -1, the return value the number of survivors.  Every owned candidate below `count` is counted, and one
// whose key is 0 never survives.  Radix select from the top byte (it stops at the first pass whose bin is taken whole), then
// one packed scan of (equal << 16 | greater), so count < 65536.  Called by all threads; hist[256] is all zero on entry and on
// return; wtot[kBeamWaves] and sel[3] are scratch.  Barriers: 2 a radix pass, 1 for the scan's totals.
template <int CPT>
__device__ __forceinline__ int beam_select(const u64 (&key)[CPT], int first, int cpt, int count, int want, int* hist, unsigned* wtot,
                                           int* sel, int lane, int wave, int (&slot)[CPT]) {
  u64 prefix = 0;
  int need = min(want, count), fshift = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
    for (int q = 0; q < CPT; ++q)
      if (q < cpt && first + q < count && (shift == 56 || (key[q] >> (shift + 8)) == (prefix >> (shift + 8))))
        atomicAdd(&hist[(int)((key[q] >> shift) & 255)], 1);
    __syncthreads();
    if (wave == 0) {      // lane l: bins 255 - 4 l down to 252 - 4 l; the bin in which the count from the top reaches `need`
      int h[4], s = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) { h[r] = hist[255 - 4 * lane - r]; hist[255 - 4 * lane - r] = 0; s += h[r]; }
      const int incl = (int)wave_scan((unsigned)s, lane);
      int r = need - (incl - s);
      if (r >= 1 && r <= s) {      // exactly one lane
        bool found = false;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (!found) {
            if (r <= h[q]) { sel[0] = 255 - 4 * lane - q; sel[1] = r; sel[2] = h[q]; found = true; }
            else r -= h[q];
          }
      }
    }
    __syncthreads();
    prefix |= (u64)sel[0] << shift;
    need = sel[1];
    fshift = shift;
    if (sel[2] == need) break;      // the bin is taken whole: no need to order it (uniform: every thread read the same words)
  }
  const u64 tp = prefix >> fshift;
  unsigned cnt = 0;
#pragma unroll
  for (int q = 0; q < CPT; ++q)
    if (q < cpt && first + q < count && key[q] != 0) {
      const u64 hp = key[q] >> fshift;
      cnt += hp > tp ? 1u : (hp == tp ? 0x10000u : 0u);
    }
  const unsigned incl = wave_scan(cnt, lane);
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  unsigned before = incl - cnt, total = 0;
#pragma unroll
  for (int w = 0; w < kBeamWaves; ++w) {
    if (w < wave) before += wtot[w];
    total += wtot[w];
  }
  int G = (int)(before & 0xFFFF), E = (int)(before >> 16);
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    int s = -1;
    if (q < cpt && first + q < count && key[q] != 0) {
      const u64 hp = key[q] >> fshift;
      if (hp > tp) { s = G + min(E, need); ++G; }
      else if (hp == tp) { if (E < need) s = G + E; ++E; }
    }
    slot[q] = s < want ? s : -1;      // (the select keeps min(want, count) at most: s < want)
  }
  return min(want, (int)(total & 0xFFFF) + min((int)(total >> 16), need));
}

// The tail of a search, by all threads behind the caller's barrier: thread j < B holds sc, the score of final slot j (-inf
// from nb on), and len / node are the final beam's arrays.  Ranks the slots by counting (ties keep the beam's order), writes
// out_scores and out_lens (-1 for an unused slot) of utterance n, walks the back-pointers of bp into the rows of out_tokens
// (`stride` words each) and pads them with -1.  s_score[B] and s_len[B] are LDS scratch.
__device__ __forceinline__ void beam_tail(double sc, int nb, int B, const int* len, const int* node, const int2* bp, int stride, int n,
                                          double* s_score, int* s_len, int32_t* out_tokens, int32_t* out_lens, double* out_scores,
                                          int tx) {
  if (tx < B) s_score[tx] = sc;
  __syncthreads();
  if (tx < B) {
    int rank = 0;
    for (int i = 0; i < B; ++i) {
      const double o = s_score[i];
      rank += (o > sc || (o == sc && i < tx)) ? 1 : 0;
    }
    const int len_j = tx < nb ? len[tx] : 0;
    out_scores[(size_t)n * B + rank] = sc;
    out_lens[(size_t)n * B + rank] = tx < nb ? len_j : -1;
    s_len[rank] = len_j;
    int32_t* o = out_tokens + ((size_t)n * B + rank) * stride;
    int nd = tx < nb ? node[tx] : 0;
    for (int d = len_j - 1; d >= 0 && nd > 0; --d) {
      const int2 e = bp[nd - 1];
      o[d] = e.y;
      nd = e.x;
    }
  }
  __syncthreads();
  for (int64_t i = tx; i < (int64_t)B * stride; i += kBeamThreads) {
    const int r = (int)(i / stride), d = (int)(i - (int64_t)r * stride);
    if (d >= s_len[r]) out_tokens[(size_t)n * B * stride + i] = -1;
  }
}

}  // namespace pk2
