// Transducer beam search for a stateless predictor of context 1 on gfx950 (include/pk2hip.h: pk2_transducer_beam_search;
// DESIGN.md 7.23).  Time-synchronous, at most R = max_symbols labels per frame.  A hypothesis is a blank-free prefix h with a
// float64 log-probability; the joint depends on (t, last(h)) only, last(()) = blank:
//
//   A = {(): 0};  for t < T_n:  Out = {};  for r = 0..R:
//     lp_h = log_softmax(z(t, last(h)))                     for h in A, float32
//     Out[h] = logadd(Out[h], A[h] + lp_h[blank])           merged by (64-bit hash, length); new entries appended in slot order
//     if r == R: break
//     cand = {h + (c,): A[h] + lp_h[c]}, c in the K non-blank columns of the largest z of row h (ties: the lower column)
//     A = the `beam` largest of cand, kept in candidate order (parent slot, then rank); ties: the lower candidate
//   A = the `beam` largest of Out, kept in the order they were made; ties: the entry made first
//
// ONE launch, one workgroup of 1024 threads per utterance over all its frames; nothing is read back, no workgroup waits on
// another, no atomics on floats.  tb_search<JOIN, VEC>:
//   additive (JOIN = false)  z(t, p) = am[t, :] + table[p, :], formed on the fly by the row pass.
//   joiner   (JOIN = true)   z(t, p) = tanhf(enc[t, :] + pred[p, :]) . w_out^T + b_out.  enc[t] sits in LDS (the next frame's row
//                            is loaded at the top of the frame and stored ahead of its last barrier).  A round's hypotheses
//                            are the 32 rows of one v_mfma_f32_32x32x2_f32 tile: all threads build H[32][Jp + 4] in LDS (zeros
//                            for odd J's pad column and the unused slots); wave w owns the column tiles w, w + 16, ... of V.
//                            The two k's of a step are j and Jp / 2 + j, so that lane (column c, half h) reads
//                            w_out[c][h Jp / 2 ...] contiguously (16-byte loads with VEC: J % 8 == 0 and aligned rows) and H
//                            likewise; the accumulator starts at b_out[c].  w_out is always streamed from L2, and a round's
//                            [32][V] logits go to a per-utterance block of the workspace that stays in L2: at J = 512,
//                            V = 1031 neither fits LDS next to H, and one route serves every shape.
// A round, barriers in brackets:
//   1 (joiner) H, the product, the logits block                                                                   [2]
//   2 row pass, a wave per hypothesis: online max and sum, lp(blank), and unless r = R, K rounds of a wave arg-max on
//     the key (ordered logit bits, ~column) below the last winner (ctcb_rows' scheme)                              [1]
//   3 a wave per hypothesis looks its prefix up in Out; every thread forms its candidate (slot i, rank k)          [1]
//   4 wave 0 merges or appends the blank moves, while all threads run tb_select, one candidate a thread: the radix
//     select of the beam-th largest candidate on the ordered bits of the doubles, 8 bits a pass from the top, LDS
//     integer histogram (ctc_beam.hip's beam_select with one candidate a thread measured 0.4 to 0.8 % slower here
//     on the additive head, profiles/beam_shared_ab.txt: this search keeps its own)                         [2 a pass]
//     then one packed scan (greater | equal) in candidate order gives every survivor its slot                      [1]
//   5 the survivors go to the other beam buffer; a new prefix writes (parent node, token) to the back-pointer table [1]
// The frame ends with the same select over Out (at most beam (R + 1) <= 1024 entries, one per thread).  The beam lives in
// LDS, double-buffered, as arrays over the slots: score, hash, length, trie node, last token (a parent's hash is not kept:
// only Out merges, and by the prefix's own identity).  The tail is beam_tail (beam_dev.h): it ranks the finals by counting
// and walks the back-pointers.
#include <algorithm>
#include <cmath>

#include "beam_dev.h"

#pragma clang fp contract(off)

namespace pk2 {
namespace {

typedef float tb_f16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = kBeamThreads;
constexpr int kWaves = kBeamWaves;
constexpr int kTile = 32;           // rows and columns of the MFMA tile
constexpr int kHPad = 4;            // floats behind a row of H
static_assert(PK2_TRANSDUCER_BEAM_MAX == kTile, "a round's hypotheses are the rows of one MFMA tile");
static_assert(PK2_TRANSDUCER_BEAM_MAX * (PK2_TRANSDUCER_BEAM_MAX_SYMBOLS + 1) <= kThreads, "one thread per entry of Out");
static_assert(PK2_TRANSDUCER_BEAM_MAX * PK2_TRANSDUCER_BEAM_MAX_TOKENS <= kThreads, "one thread per candidate");
static_assert(PK2_TRANSDUCER_BEAM_MAX_JOIN <= kThreads, "one thread per column of enc[t]");

struct TbParams {
  const int32_t* lengths;
  const float *x, *rows, *w, *bias;
  int64_t ss, fs, rs, wstr;
  int32_t Tpad, V, Vs, J, Jp, blank, B, K, R;
  float* logits;      // [N][32][Vs] (joiner)
  int2* bp;           // [N][Tpad R B]
  int32_t *out_tokens, *out_lens, *out_status;
  double* out_scores;
};

// The LDS of tb_search in bytes from its base (every array on a 16-byte boundary).
struct TbLds {
  size_t score, hash, node, last, len, o_score, o_hash, o_node, o_last, o_len, tokc, toklp, lpb, match, enc, h, bytes;
};
__host__ __device__ inline TbLds tb_lds(size_t B, size_t K, size_t R, size_t Jp) {
  TbLds l;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t r = o; o += (n + 15) / 16 * 16; return r; };
  const size_t cap = B * (R + 1);
  l.score = take(16 * B); l.hash = take(16 * B); l.node = take(8 * B); l.last = take(8 * B); l.len = take(8 * B);      // [2][B]
  l.o_score = take(8 * cap); l.o_hash = take(8 * cap); l.o_node = take(4 * cap); l.o_last = take(4 * cap); l.o_len = take(4 * cap);
  l.tokc = take(4 * B * K); l.toklp = take(4 * B * K); l.lpb = take(4 * B); l.match = take(4 * B);
  l.enc = take(8 * Jp);                                         // [2][Jp]
  l.h = take(Jp ? 4 * kTile * (Jp + kHPad) : 0);
  l.bytes = o;
  return l;
}

__device__ __forceinline__ int tb_wave_max_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// The slot of this thread's candidate among the `want` largest keys of the `count` valid ones, survivors in thread order, or -1;
// kept = the number of survivors.  Radix select from the top byte (it stops at the first pass whose bin is taken whole), then
// one packed scan of (equal << 16 | greater).  Called by all threads; hist is all zero on entry and on return.
__device__ __forceinline__ int tb_select(bool valid, u64 key, int count, int want, int* hist, unsigned* wtot, int* sel, int lane, int wave,
                                         int& kept) {
  u64 prefix = 0;
  int need = min(want, count), fshift = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (valid && (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
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
  const u64 tp = prefix >> fshift, hp = key >> fshift;
  const unsigned cnt = !valid ? 0u : (hp > tp ? 1u : (hp == tp ? 0x10000u : 0u));
  const unsigned incl = wave_scan(cnt, lane);
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  unsigned before = incl - cnt, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) before += wtot[w];
    total += wtot[w];
  }
  const int G = (int)(before & 0xFFFF), E = (int)(before >> 16);
  kept = min(want, (int)(total & 0xFFFF) + min((int)(total >> 16), need));
  int s = -1;
  if (cnt == 1u) s = G + min(E, need);
  else if (cnt != 0u && E < need) s = G + E;
  return s < want ? s : -1;      // (the select keeps min(want, count) at most: s < want)
}

// ---- tb_search: grid (N), tb_lds(B, K, R, Jp).bytes of dynamic LDS.
template <bool JOIN, bool VEC>
__global__ __launch_bounds__(kThreads) void tb_search(const TbParams p) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int hist[256];
  __shared__ unsigned wtot[kWaves];
  __shared__ int sel[3];
  __shared__ int bad;
  const int n = blockIdx.x, tx = threadIdx.x, lane = tx & 63, wave = tx >> 6;
  const int B = p.B, K = p.K, R = p.R, V = p.V, J = p.J, Jp = p.Jp, T = min(p.lengths[n], p.Tpad);
  const TbLds L = tb_lds(B, K, R, Jp);
  double* score = reinterpret_cast<double*>(lds + L.score);
  u64* hash = reinterpret_cast<u64*>(lds + L.hash);
  int* node = reinterpret_cast<int*>(lds + L.node);
  int* last = reinterpret_cast<int*>(lds + L.last);
  int* len = reinterpret_cast<int*>(lds + L.len);
  double* o_score = reinterpret_cast<double*>(lds + L.o_score);
  u64* o_hash = reinterpret_cast<u64*>(lds + L.o_hash);
  int* o_node = reinterpret_cast<int*>(lds + L.o_node);
  int* o_last = reinterpret_cast<int*>(lds + L.o_last);
  int* o_len = reinterpret_cast<int*>(lds + L.o_len);
  int* tokc = reinterpret_cast<int*>(lds + L.tokc);
  float* toklp = reinterpret_cast<float*>(lds + L.toklp);
  float* lpb = reinterpret_cast<float*>(lds + L.lpb);
  int* match = reinterpret_cast<int*>(lds + L.match);
  float* encb = reinterpret_cast<float*>(lds + L.enc);
  float* H = reinterpret_cast<float*>(lds + L.h);
  const int HS = Jp + kHPad, J2 = Jp >> 1;

  if (tx == 0) {      // the empty prefix in slot 0 of buffer 0
    score[0] = 0.0; hash[0] = kHashEmpty; node[0] = 0; last[0] = p.blank; len[0] = 0;
    bad = 0;
  }
  if (tx < 256) hist[tx] = 0;
  const float* xg = p.x + (int64_t)n * p.ss;
  float* zl = p.logits + (size_t)n * kTile * p.Vs;
  int2* bp = p.bp + (size_t)n * p.Tpad * R * B;
  if (JOIN && T > 0 && tx < Jp) encb[tx] = tx < J ? xg[tx] : 0.f;
  int nb = 1, cur = 0, nout = 0;
  bool numeric = false;
  __syncthreads();

  for (int t = 0; t < T && !numeric; ++t) {
    const float* xt = xg + (int64_t)t * p.fs;
    const float* enc = encb + (t & 1) * Jp;
    float nxt = 0.f;
    if (JOIN && t + 1 < T && tx < J) nxt = xt[p.fs + tx];
    for (int r = 0; r <= R; ++r) {
      const int co = cur * B, no = (cur ^ 1) * B;
      if (JOIN) {
        // 1: the hidden rows, then the [32][V] logits of the round
        for (int e = tx; e < kTile * Jp; e += kThreads) {
          const int i = e / Jp, j = e - i * Jp;
          float h = 0.f;
          if (i < nb && j < J) h = tanhf(enc[j] + p.rows[(int64_t)last[co + i] * p.rs + j]);
          H[i * HS + j] = h;
        }
        __syncthreads();
        const int half = lane >> 5, cl = lane & 31;
        for (int tile = wave; tile * kTile < V; tile += kWaves) {
          const int col = min(tile * kTile + cl, V - 1);      // (the columns past V repeat the last one and are not read back)
          const float* wrow = p.w + (int64_t)col * p.wstr + half * J2;
          const float* arow = H + cl * HS + half * J2;
          const float b0 = p.bias[col];
          tb_f16 acc;
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[v] = b0;
          if (VEC) {
            for (int kk = 0; kk < J2; kk += 4) {
              const float4 b = *reinterpret_cast<const float4*>(wrow + kk);
              const float4 a = *reinterpret_cast<const float4*>(arow + kk);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
            }
          } else {
            for (int kk = 0; kk < J2; ++kk) {
              const float b = half * J2 + kk < J ? wrow[kk] : 0.f;      // (odd J: the pad column is not in w_out)
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[kk], b, acc, 0, 0, 0);
            }
          }
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int row = (v & 3) + 8 * (v >> 2) + 4 * half;
            if (row < nb) zl[(size_t)row * p.Vs + tile * kTile + cl] = acc[v];
          }
        }
        block_sync_global();
      }
      // 2: the row pass
      for (int i = wave; i < nb; i += kWaves) {
        const float* za = JOIN ? zl + (size_t)i * p.Vs : xt;
        const float* zb = p.rows + (int64_t)last[co + i] * p.rs;
        auto z = [&](int v) { return JOIN ? za[v] : za[v] + zb[v]; };
        float m = -INFINITY, s = 0.f;
        for (int v = lane; v < V; v += 64) {
          const float q = z(v), mn = fmaxf(m, q);
          const float keep = m == -INFINITY ? 0.f : __expf(m - mn), add = q == -INFINITY ? 0.f : __expf(q - mn);
          s = s * keep + add;
          m = mn;
        }
        const float M = wave_max(m);
        s = m == -INFINITY ? 0.f : s * __expf(m - M);
        const float Z = wave_sum(s);
        if (!(isfinite(M) && isfinite(Z))) {
          if (lane == 0) bad = 1;
          continue;
        }
        const float logz = logf(Z);
        if (lane == 0) lpb[i] = (z(p.blank) - M) - logz;
        if (r == R) continue;
        u64 prev = ~0ull;      // K rounds: the largest key below the last winner, over this lane's columns and then over the wave
        for (int k = 0; k < K; ++k) {
          u64 best = 0;
          for (int v = lane; v < V; v += 64) {
            const u64 key = beam_key(z(v), v);
            if (v != p.blank && key < prev && key > best) best = key;
          }
          best = wave_max64(best);
          prev = best;
          int col = beam_key_col(best);
          if (col < 0 || col >= V) col = p.blank;      // (K <= V - 1 columns exist: not taken)
          if (lane == 0) {
            tokc[i * K + k] = col;
            toklp[i * K + k] = (z(col) - M) - logz;
          }
        }
      }
      __syncthreads();
      if (bad) { numeric = true; break; }      // uniform: every thread read the same word
      // 3: where each hypothesis is in Out, and this thread's candidate
      for (int i = wave; i < nb; i += kWaves) {
        const u64 hh = hash[co + i];
        const int ll = len[co + i];
        int found = -1;
        for (int e = lane; e < nout; e += 64)
          if (o_hash[e] == hh && o_len[e] == ll) found = e;
        found = tb_wave_max_int(found);
        if (lane == 0) match[i] = found;
      }
      const int ncand = nb * K;
      const bool valid = r < R && tx < ncand;
      const int ci = valid ? tx / K : 0;
      const double cs = valid ? score[co + ci] + (double)toklp[tx] : 0.0;
      __syncthreads();
      // 4: the blank moves into Out, merged or appended in slot order
      const bool fresh = lane < nb && match[lane] < 0;
      const u64 freshmask = __ballot(fresh);
      if (wave == 0 && lane < nb) {
        const double v = score[co + lane] + (double)lpb[lane];
        const int mt = match[lane];
        if (mt >= 0) {
          o_score[mt] = log_add(o_score[mt], v);
        } else {
          const int e = nout + __popcll(freshmask & ((1ull << lane) - 1ull));
          o_score[e] = v; o_hash[e] = hash[co + lane]; o_node[e] = node[co + lane]; o_last[e] = last[co + lane]; o_len[e] = len[co + lane];
        }
      }
      nout += __popcll(freshmask);
      if (r == R) break;
      // 5: the beam-th largest candidate, the survivors into the other buffer
      int kept;
      const int s = tb_select(valid, beam_ordered(cs), ncand, B, hist, wtot, sel, lane, wave, kept);
      if (s >= 0) {
        const int c = tokc[tx], nd = 1 + (t * R + r) * B + s;
        score[no + s] = cs; hash[no + s] = beam_mix(hash[co + ci], c); node[no + s] = nd; last[no + s] = c; len[no + s] = len[co + ci] + 1;
        bp[nd - 1] = make_int2(node[co + ci], c);
      }
      nb = kept;
      cur ^= 1;
      __syncthreads();
    }
    if (numeric) break;
    __syncthreads();
    // the frame's cut: the `beam` largest of Out
    {
      const int no = (cur ^ 1) * B;
      const bool valid = tx < nout;
      int kept;
      const int s = tb_select(valid, beam_ordered(valid ? o_score[tx] : 0.0), nout, B, hist, wtot, sel, lane, wave, kept);
      if (s >= 0) {
        score[no + s] = o_score[tx]; hash[no + s] = o_hash[tx]; node[no + s] = o_node[tx]; last[no + s] = o_last[tx]; len[no + s] = o_len[tx];
      }
      if (JOIN && t + 1 < T && tx < Jp) encb[((t + 1) & 1) * Jp + tx] = nxt;
      nb = kept;
      cur ^= 1;
      nout = 0;
      __syncthreads();
    }
  }

  // tail: the order of the scores (ties keep the beam's), the token sequences from the back-pointers
  block_sync_global();
  const int co = cur * B;
  if (numeric) nb = 0;
  const double sc = tx < nb ? score[co + tx] : -INFINITY;
  if (tx == 0) p.out_status[n] = numeric ? PK2_TRANSDUCER_NUMERIC : PK2_TRANSDUCER_OK;
  beam_tail(sc, nb, B, len + co, node + co, bp, p.Tpad * R, n, o_score, o_len, p.out_tokens, p.out_lens, p.out_scores, tx);
}

size_t tb_logit_bytes(int64_t N, int V, int J) { return J > 0 ? align_up((size_t)N * kTile * align_up((size_t)V, kTile) * 4, 256) : 0; }

template <bool JOIN, bool VEC>
int tb_launch(const TbParams& p, int N, size_t lds, hipStream_t stream) {
  if (lds > 64 * 1024)
    PK2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&tb_search<JOIN, VEC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((tb_search<JOIN, VEC>), dim3(N), dim3(kThreads), lds, stream, p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

}  // namespace
}  // namespace pk2

using namespace pk2;

extern "C" size_t pk2_transducer_beam_workspace_bytes(int32_t num_utts, int32_t T, int32_t num_classes, int32_t beam, int32_t max_symbols,
                                                      int32_t join_dim) {
  if (num_utts < 1 || T < 0 || num_classes < 2 || beam < 1 || beam > PK2_TRANSDUCER_BEAM_MAX || max_symbols < 1 ||
      max_symbols > PK2_TRANSDUCER_BEAM_MAX_SYMBOLS || join_dim < 0 || join_dim > PK2_TRANSDUCER_BEAM_MAX_JOIN)
    return 0;
  return tb_logit_bytes(num_utts, num_classes, join_dim) + align_up((size_t)num_utts * T * max_symbols * beam * sizeof(int2), 256) + 256;
}

extern "C" int pk2_transducer_beam_search(const int32_t* lengths, const int32_t* lengths_dev, int32_t num_utts, const float* x,
                                          int64_t seq_stride, int64_t frame_stride, int32_t T, const float* rows, int64_t rows_stride,
                                          const float* w_out, int64_t w_stride, const float* b_out, int32_t join_dim, int32_t num_classes,
                                          int32_t blank, int32_t beam, int32_t top_tokens, int32_t max_symbols, int32_t* out_tokens,
                                          int32_t* out_lens, double* out_scores, int32_t* out_status, void* workspace, size_t workspace_bytes,
                                          void* stream_) {
  PK2_REQUIRE(lengths && lengths_dev && rows && out_lens && out_scores && out_status && workspace, "pk2_transducer_beam_search: null argument");
  PK2_REQUIRE(num_utts >= 1 && T >= 0 && seq_stride >= 0 && frame_stride >= 0 && rows_stride >= 0 && w_stride >= 0,
              "transducer beam search: %d utterances of %d frames, bad strides", num_utts, T);
  PK2_REQUIRE(T == 0 || (x && out_tokens), "pk2_transducer_beam_search: null argument");
  PK2_REQUIRE(num_classes >= 2 && blank >= 0 && blank < num_classes, "transducer beam search: blank %d of %d columns", blank, num_classes);
  PK2_REQUIRE(join_dim >= 0 && (join_dim == 0 || (w_out && b_out)), "transducer beam search: join_dim %d, or a joiner without w_out / b_out",
              join_dim);
  if (beam < 1 || beam > PK2_TRANSDUCER_BEAM_MAX || top_tokens < 1 || top_tokens > PK2_TRANSDUCER_BEAM_MAX_TOKENS || max_symbols < 1 ||
      max_symbols > PK2_TRANSDUCER_BEAM_MAX_SYMBOLS || join_dim > PK2_TRANSDUCER_BEAM_MAX_JOIN) {
    set_error("transducer beam search: beam %d (1..%d), top_tokens %d (1..%d), max_symbols %d (1..%d), join_dim %d (..%d)", beam,
              PK2_TRANSDUCER_BEAM_MAX, top_tokens, PK2_TRANSDUCER_BEAM_MAX_TOKENS, max_symbols, PK2_TRANSDUCER_BEAM_MAX_SYMBOLS, join_dim,
              PK2_TRANSDUCER_BEAM_MAX_JOIN);
    return PK2_ERR_LIMIT;
  }
  if ((int64_t)T * max_symbols * beam >= ((int64_t)1 << 31) - 1) {
    set_error("transducer beam search: %d frames x %d symbols x beam %d node ids do not fit 31 bits", T, max_symbols, beam);
    return PK2_ERR_LIMIT;
  }
  for (int32_t n = 0; n < num_utts; ++n)
    PK2_REQUIRE(lengths[n] >= 0 && lengths[n] <= T, "transducer beam search: utterance %d has %d frames, the tensor %d", n, lengths[n], T);
  const size_t need = pk2_transducer_beam_workspace_bytes(num_utts, T, num_classes, beam, max_symbols, join_dim);
  PK2_REQUIRE(workspace_bytes >= need, "transducer beam search: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  PK2_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "transducer beam search: the workspace must be 256-byte aligned");
  TbParams p;
  memset(&p, 0, sizeof(p));
  p.lengths = lengths_dev; p.x = x; p.rows = rows; p.w = w_out; p.bias = b_out;
  p.ss = seq_stride; p.fs = frame_stride; p.rs = rows_stride; p.wstr = w_stride;
  p.Tpad = T; p.V = num_classes; p.Vs = (int32_t)align_up((size_t)num_classes, kTile); p.J = join_dim; p.Jp = (join_dim + 1) & ~1;
  p.blank = blank; p.B = beam; p.K = std::min(top_tokens, num_classes - 1); p.R = max_symbols;
  p.logits = static_cast<float*>(workspace);
  p.bp = reinterpret_cast<int2*>(static_cast<char*>(workspace) + tb_logit_bytes(num_utts, num_classes, join_dim));
  p.out_tokens = out_tokens; p.out_lens = out_lens; p.out_scores = out_scores; p.out_status = out_status;
  const size_t lds = tb_lds(p.B, p.K, p.R, p.Jp).bytes;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (join_dim == 0) return tb_launch<false, false>(p, num_utts, lds, stream);
  const bool vec = join_dim % 8 == 0 && (reinterpret_cast<uintptr_t>(w_out) & 15) == 0 && w_stride % 4 == 0;
  return vec ? tb_launch<true, true>(p, num_utts, lds, stream) : tb_launch<true, false>(p, num_utts, lds, stream);
}
