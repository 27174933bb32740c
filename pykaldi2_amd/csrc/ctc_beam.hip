// CTC prefix beam search with shallow fusion of a backoff n-gram LM on gfx950 (include/pk2hip.h: pk2_ctc_beam_search;
// DESIGN.md 7.20).  A hypothesis is a blank-free prefix l with two masses, pb(l) / pnb(l): the probability of the alignments of
// the frames so far that collapse to l and end in blank / in a non-blank, times the LM factor of l.  Frame t, with
// y = softmax(x[t, .]) and C_t the K non-blank columns of the largest logit:
//
//   stay    pb'(l)  += y(blank) (pb(l) + pnb(l))          pnb'(l) += y(last(l)) pnb(l)
//   extend  pnb'(l + c) += y(c) f(c | l) (pb(l) + [c != last(l)] pnb(l)),  c in C_t,  f = exp(-lm_weight cost + bonus)
//   merge   an extension l + c that is itself in the beam lands on that hypothesis
//   prune   the `beam` largest pb' + pnb' > 0 survive; ties: stays first, then the lower parent slot, then the rank in C_t
//
// Two launches on one stream, nothing is read back, no workgroup waits on another, no atomics on floats:
//   ctcb_rows    a wave per frame, the only pass over T x P: online max and sum over 16-byte loads, then K rounds of a wave
//                arg-max on the key (ordered logit bits, ~column) below the last winner.  Writes the compact row
//                {m, 1 / Z, y(blank), 0, K x (column, y(column))} in rank order.
//   ctcb_search  one workgroup of 1024 threads per utterance, all frames.  The beam lives in LDS, double-buffered, as arrays
//                over the slots: pb, pnb (f64), the hash of the prefix and of its parent, its length, trie node (the index of
//                its back-pointer), last token, LM state.  A prefix is identified by (64-bit hash, length): node ids cannot
//                serve, a prefix that was pruned and made again has a new one.  Per frame (barriers in brackets):
//                  1 a thread per slot j finds the slot of its parent and the rank of its last token: redir[i][k] = j [1]
//                  2 the nb K extensions over all threads, one LM lookup each; a redirected one goes to mval[j]       [1]
//                  3 a thread per slot: the stay candidate, plus mval[j]                                              [1]
//                  4 beam_select (beam_dev.h) with up to 5 candidates a thread: radix select of the beam-th largest
//                    total on the bits of the positive doubles, 8 bits a pass from the top, LDS integer histogram; it
//                    stops at the first pass whose bin is taken whole                                           [2 a pass]
//                    then one packed scan (greater | equal) in candidate order gives every survivor its slot          [1]
//                  5 the survivors are written to the other beam buffer times 2^-e, e the exponent of the best total
//                    (exact; the integer sum of the e is the log scale), new prefixes write (parent node, token) to
//                    the table                                                                                        [1]
//                The next compact row is loaded at the top of the frame and stored ahead of its last barrier.  The tail
//                takes log once per slot and adds the </s> cost; beam_tail (beam_dev.h) ranks the finals by counting
//                and walks the back-pointers.  The LM lookup is ngram_arc (ngram_dev.h).
#include <algorithm>
#include <cmath>

#include "beam_dev.h"
#include "ngram_dev.h"

#pragma clang fp contract(off)

namespace pk2 {
namespace {

constexpr int kThreads = kBeamThreads;
constexpr int kWaves = kBeamWaves;
constexpr int kMaxCand = PK2_CTC_BEAM_MAX * (PK2_CTC_BEAM_MAX_TOKENS + 1);      // 4224
constexpr int kMaxCpt = (kMaxCand + kThreads - 1) / kThreads;                    // 5 candidates per thread at the limits
constexpr int kRowHead = 4;
constexpr unsigned kNone = 0xFF;
static_assert(PK2_CTC_BEAM_MAX <= 255 && kMaxCand < 65536, "redir is a byte, the scan packs two 16-bit counts");

__host__ __device__ inline int cb_row_words(int K) { return kRowHead + 2 * K; }

struct CbParams {
  const int32_t* lengths;
  const float* x;
  int64_t ss, fs;
  int32_t Tpad, P, blank, B, K;
  NgramTrie lm;
  const int32_t* lm_ids;
  int32_t lm_start, lm_eos, has_lm, use_eos;
  double lm_weight, bonus;
  float* rows;
  int2* bp;
  int32_t *out_tokens, *out_lens, *out_status;
  double* out_scores;
};

// The LDS of ctcb_search in bytes from its base, for beam B and K tokens (every array on an 8-byte boundary).
struct CbLds {
  size_t pb, pnb, hash, phash, node, last, lm, len, stay_pb, stay_pnb, mval, src, key, extlm, redir, row, bytes;
};
__host__ __device__ inline CbLds cb_lds(size_t B, size_t K) {
  CbLds l;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t r = o; o += (n + 7) / 8 * 8; return r; };
  l.pb = take(16 * B); l.pnb = take(16 * B); l.hash = take(16 * B); l.phash = take(16 * B);      // [2][B], the two beam buffers
  l.node = take(8 * B); l.last = take(8 * B); l.lm = take(8 * B); l.len = take(8 * B);
  l.stay_pb = take(8 * B); l.stay_pnb = take(8 * B); l.mval = take(8 * B); l.src = take(4 * B);
  l.key = take(8 * B * (K + 1)); l.extlm = take(4 * B * K); l.redir = take(B * K);
  l.row = take(8 * cb_row_words(K));                                                              // [2][row words]
  l.bytes = o;
  return l;
}

// ---- ctcb_rows: grid (blocks, N), a wave per frame.
__global__ __launch_bounds__(256) void ctcb_rows(const int32_t* __restrict__ lengths, const float* __restrict__ x, int64_t seq_stride,
                                                 int64_t frame_stride, int32_t Tpad, int32_t P, int32_t blank, int32_t K,
                                                 float* __restrict__ rows) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int T = min(lengths[n], Tpad), RW = cb_row_words(K);
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  for (int t = wave; t < T; t += nwaves) {
    const float* row = x + (int64_t)n * seq_stride + (int64_t)t * frame_stride;
    // the row as [head scalars][16-byte aligned float4s][tail scalars]; the scalars are at most 6, one lane each
    const int head = min(P, (int)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) >> 2));
    const int nvec = (P - head) >> 2, tail0 = head + 4 * nvec;
    const int mine = lane < head ? lane : (lane < head + P - tail0 ? tail0 + lane - head : -1);      // this lane's scalar column
    float m = -INFINITY, s = 0.f;
    for (int v = lane; v < nvec; v += 64) {
      const float4 q = *reinterpret_cast<const float4*>(row + head + 4 * v);
      const float mn = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
      const float part = (__expf(q.x - mn) + __expf(q.y - mn)) + (__expf(q.z - mn) + __expf(q.w - mn));
      s = s * __expf(m - mn) + part;
      m = mn;
    }
    if (mine >= 0) {
      const float v = row[mine];
      const float mn = fmaxf(m, v);
      s = s * __expf(m - mn) + __expf(v - mn);
      m = mn;
    }
    const float M = wave_max(m);
    s = s * __expf(m - M);                      // a lane without an element has s = 0, m = -inf: 0 * 0
    const float inv = 1.f / wave_sum(s);
    float* out = rows + ((size_t)n * Tpad + t) * RW;
    if (lane == 0) {
      out[0] = M;
      out[1] = inv;
      out[2] = __expf(row[blank] - M) * inv;
      out[3] = 0.f;
    }
    // K rounds: the largest key below the last winner, over this lane's elements and then over the wave
    u64 prev = ~0ull;
    for (int k = 0; k < K; ++k) {
      u64 best = 0;
      auto consider = [&](float v, int col) {
        const u64 key = beam_key(v, col);
        if (col != blank && key < prev && key > best) best = key;
      };
      for (int v = lane; v < nvec; v += 64) {
        const float4 q = *reinterpret_cast<const float4*>(row + head + 4 * v);
        const int c = head + 4 * v;
        consider(q.x, c); consider(q.y, c + 1); consider(q.z, c + 2); consider(q.w, c + 3);
      }
      if (mine >= 0) consider(row[mine], mine);
      best = wave_max64(best);
      prev = best;
      int col = beam_key_col(best);
      if (col < 0 || col >= P) col = blank;      // (K <= P - 1 columns exist: not taken)
      if (lane == 0) {
        out[kRowHead + 2 * k] = __int_as_float(col);
        out[kRowHead + 2 * k + 1] = __expf(row[col] - M) * inv;
      }
    }
  }
}

// ---- ctcb_search: grid (N), cb_lds(B, K).bytes of dynamic LDS.
__global__ __launch_bounds__(kThreads) void ctcb_search(const CbParams p) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int hist[256];
  __shared__ u64 wmax[kWaves];
  __shared__ unsigned wtot[kWaves];
  __shared__ int sel[3];
  const int n = blockIdx.x, tx = threadIdx.x, lane = tx & 63, wave = tx >> 6;
  const int B = p.B, K = p.K, RW = cb_row_words(K), T = min(p.lengths[n], p.Tpad);
  const CbLds L = cb_lds(B, K);
  double* pb = reinterpret_cast<double*>(lds + L.pb);
  double* pnb = reinterpret_cast<double*>(lds + L.pnb);
  u64* hash = reinterpret_cast<u64*>(lds + L.hash);
  u64* phash = reinterpret_cast<u64*>(lds + L.phash);
  int* node = reinterpret_cast<int*>(lds + L.node);
  int* last = reinterpret_cast<int*>(lds + L.last);
  int* lms = reinterpret_cast<int*>(lds + L.lm);
  int* len = reinterpret_cast<int*>(lds + L.len);
  double* stay_pb = reinterpret_cast<double*>(lds + L.stay_pb);
  double* stay_pnb = reinterpret_cast<double*>(lds + L.stay_pnb);
  double* mval = reinterpret_cast<double*>(lds + L.mval);
  int* src = reinterpret_cast<int*>(lds + L.src);
  u64* key = reinterpret_cast<u64*>(lds + L.key);
  int* extlm = reinterpret_cast<int*>(lds + L.extlm);
  unsigned char* redir = lds + L.redir;
  float* rowbuf = reinterpret_cast<float*>(lds + L.row);

  if (tx == 0) {      // the empty prefix in slot 0 of buffer 0
    pb[0] = 1.0; pnb[0] = 0.0; hash[0] = kHashEmpty; phash[0] = 0; node[0] = 0; last[0] = -1; lms[0] = p.lm_start; len[0] = 0;
  }
  for (int e = tx; e < B * K; e += kThreads) redir[e] = kNone;
  if (tx < 256) hist[tx] = 0;
  const float* rowg = p.rows + (size_t)n * p.Tpad * RW;
  int2* bp = p.bp + (size_t)n * p.Tpad * B;
  if (T > 0 && tx < RW) rowbuf[tx] = rowg[tx];
  int nb = 1, cur = 0;
  long long expo = 0;      // the beam is the true masses times 2^-expo
  bool numeric = false;
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const float* row = rowbuf + (t & 1) * RW;
    const int co = cur * B, no = (cur ^ 1) * B;
    float nxt = 0.f;
    if (t + 1 < T && tx < RW) nxt = rowg[(size_t)(t + 1) * RW + tx];
    // 1: merges.  Slot j's prefix is parent + token: if the parent is in the beam and the token in C_t, that extension is j
    float xl = 0.f;
    int mysrc = -1;
    if (tx < nb && last[co + tx] >= 0) {
      const int lt = last[co + tx], ln = len[co + tx] - 1;
      const u64 ph = phash[co + tx];
      xl = p.x[(int64_t)n * p.ss + (int64_t)t * p.fs + lt];
      int pi = -1, pk = -1;
      for (int i = 0; i < nb; ++i)
        if (hash[co + i] == ph && len[co + i] == ln) pi = i;
      for (int k = 0; k < K; ++k)
        if (__float_as_int(row[kRowHead + 2 * k]) == lt) pk = k;
      if (pi >= 0 && pk >= 0) {
        mysrc = pi * K + pk;
        redir[mysrc] = (unsigned char)tx;
      }
    }
    __syncthreads();
    // 2: the extensions, candidate nb + i K + k
    const int next = nb * K, M = nb + next;
    for (int e = tx; e < next; e += kThreads) {
      const int i = e / K, k = e - i * K;
      const int c = __float_as_int(row[kRowHead + 2 * k]);
      const float y = row[kRowHead + 2 * k + 1];
      double f = 1.0;
      int hn = 0;
      bool ok = true;
      if (p.has_lm) {
        double cost;
        ok = ngram_arc(p.lm, lms[co + i], p.lm_ids ? p.lm_ids[c] : c, cost, hn);
        f = exp(-p.lm_weight * cost + p.bonus);
      }
      const double mass = pb[co + i] + (c != last[co + i] ? pnb[co + i] : 0.0);
      const double v = ok ? ((double)y * f) * mass : 0.0;
      const unsigned j = redir[e];
      if (j != kNone) {
        mval[j] = v;
        key[nb + e] = 0;
      } else {
        key[nb + e] = (u64)__double_as_longlong(v);
      }
      extlm[e] = hn;
    }
    __syncthreads();
    // 3: the stays, candidate j
    if (tx < nb) {
      const double a = pb[co + tx], b = pnb[co + tx];
      const double pbn = (double)row[2] * (a + b);
      double pnbn = 0.0;
      if (last[co + tx] >= 0) pnbn = (double)(__expf(xl - row[0]) * row[1]) * b;
      if (mysrc >= 0) {
        pnbn += mval[tx];
        redir[mysrc] = kNone;
      }
      stay_pb[tx] = pbn;
      stay_pnb[tx] = pnbn;
      key[tx] = (u64)__double_as_longlong(pbn + pnbn);
    }
    __syncthreads();
    // 4: the B largest totals (a redirected or zero-mass extension has key 0: counted, never kept).  A thread owns cpt
    // consecutive candidates, so that the slots are in candidate order.  The best total, for the rescale, goes to wmax
    // ahead of the select and is read behind its barriers: on a frame whose best total is 0 or not finite the select
    // still runs to its end (integers only, hist is zero again) and the frame breaks behind it
    const int cpt = (M + kThreads - 1) / kThreads, c0 = tx * cpt;
    u64 kq[kMaxCpt], lmax = 0;
#pragma unroll
    for (int q = 0; q < kMaxCpt; ++q) {
      kq[q] = (q < cpt && c0 + q < M) ? key[c0 + q] : 0;
      lmax = kq[q] > lmax ? kq[q] : lmax;
    }
    lmax = wave_max64(lmax);
    if (lane == 0) wmax[wave] = lmax;
    int slot[kMaxCpt];
    const int kept = beam_select<kMaxCpt>(kq, c0, cpt, M, B, hist, wtot, sel, lane, wave, slot);
    u64 best = wmax[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = wmax[w] > best ? wmax[w] : best;
    int eb = (int)((best >> 52) & 0x7FF);
    if (best == 0 || (best >> 63) || eb == 0x7FF) { numeric = true; nb = 0; break; }      // uniform: every thread read the same words
    eb = min(max(eb, 1), 2045);
    const double scale = __longlong_as_double((long long)(2046 - eb) << 52);      // 2^-(eb - 1023)
    expo += eb - 1023;
    // 5: the survivors into the other buffer
#pragma unroll
    for (int q = 0; q < kMaxCpt; ++q) {
      const int s = slot[q];
      if (s >= 0) {
        const int idx = c0 + q;
        if (idx < nb) {
          pb[no + s] = stay_pb[idx] * scale; pnb[no + s] = stay_pnb[idx] * scale;
          hash[no + s] = hash[co + idx]; phash[no + s] = phash[co + idx]; node[no + s] = node[co + idx];
          last[no + s] = last[co + idx]; lms[no + s] = lms[co + idx]; len[no + s] = len[co + idx];
        } else {
          const int e = idx - nb, i = e / K, k = e - i * K;
          const int c = __float_as_int(row[kRowHead + 2 * k]);
          pb[no + s] = 0.0; pnb[no + s] = __longlong_as_double((long long)kq[q]) * scale;
          hash[no + s] = beam_mix(hash[co + i], c); phash[no + s] = hash[co + i]; node[no + s] = 1 + t * B + s;
          last[no + s] = c; lms[no + s] = extlm[e]; len[no + s] = len[co + i] + 1;
          bp[(size_t)t * B + s] = make_int2(node[co + i], c);
        }
      }
    }
    if (t + 1 < T && tx < RW) rowbuf[((t + 1) & 1) * RW + tx] = nxt;
    nb = kept;
    cur ^= 1;
    __syncthreads();
  }

  // tail: scores, their order (ties keep the beam's), the token sequences from the back-pointers
  block_sync_global();
  const int co = cur * B;
  double sc = -INFINITY;
  if (tx < nb) {
    sc = log(pb[co + tx] + pnb[co + tx]) + (double)expo * 0.6931471805599453;
    if (p.has_lm && p.use_eos) {
      double cost;
      int hn;
      ngram_arc(p.lm, lms[co + tx], p.lm_eos, cost, hn);
      sc += -(p.lm_weight * cost);
    }
  }
  if (tx == 0) p.out_status[n] = numeric ? PK2_CTC_NUMERIC : PK2_CTC_OK;
  beam_tail(sc, nb, B, len + co, node + co, bp, p.Tpad, n, stay_pb, src, p.out_tokens, p.out_lens, p.out_scores, tx);
}

size_t cb_rows_bytes(int64_t N, int64_t T, int K) { return align_up((size_t)(N * T) * cb_row_words(K) * 4, 256); }

}  // namespace
}  // namespace pk2

using namespace pk2;

extern "C" size_t pk2_ctc_beam_workspace_bytes(int32_t num_utts, int32_t T, int32_t num_classes, int32_t beam, int32_t top_tokens) {
  if (num_utts < 1 || T < 0 || num_classes < 2 || beam < 1 || beam > PK2_CTC_BEAM_MAX || top_tokens < 1 ||
      top_tokens > PK2_CTC_BEAM_MAX_TOKENS)
    return 0;
  const int K = std::min(top_tokens, num_classes - 1);
  return cb_rows_bytes(num_utts, T, K) + align_up((size_t)num_utts * T * beam * sizeof(int2), 256) + 256;
}

extern "C" int pk2_ctc_beam_search(const int32_t* lengths, const int32_t* lengths_dev, int32_t num_utts, const float* logits,
                                   int64_t seq_stride, int64_t frame_stride, int32_t T, int32_t num_classes, int32_t blank, int32_t beam,
                                   int32_t top_tokens, const void* lm_, const int32_t* lm_ids, double lm_weight, double insertion_bonus,
                                   int32_t lm_eos, int32_t* out_tokens, int32_t* out_lens, double* out_scores, int32_t* out_status,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
  PK2_REQUIRE(lengths && lengths_dev && out_lens && out_scores && out_status && workspace, "pk2_ctc_beam_search: null argument");
  PK2_REQUIRE(num_utts >= 1 && T >= 0 && seq_stride >= 0 && frame_stride >= 0, "ctc beam search: %d utterances of %d frames, bad strides",
              num_utts, T);
  PK2_REQUIRE(T == 0 || (logits && out_tokens), "pk2_ctc_beam_search: null argument");
  PK2_REQUIRE(num_classes >= 2 && blank >= 0 && blank < num_classes, "ctc beam search: blank %d of %d columns", blank, num_classes);
  if (beam < 1 || beam > PK2_CTC_BEAM_MAX || top_tokens < 1 || top_tokens > PK2_CTC_BEAM_MAX_TOKENS) {
    set_error("ctc beam search: beam %d (1..%d), top_tokens %d (1..%d)", beam, PK2_CTC_BEAM_MAX, top_tokens, PK2_CTC_BEAM_MAX_TOKENS);
    return PK2_ERR_LIMIT;
  }
  if ((int64_t)T * beam >= ((int64_t)1 << 31) - 1) {
    set_error("ctc beam search: %d frames x beam %d node ids do not fit 31 bits", T, beam);
    return PK2_ERR_LIMIT;
  }
  const NgramDev* lm = static_cast<const NgramDev*>(lm_);
  PK2_REQUIRE(lm || !lm_ids, "ctc beam search: lm_ids without an LM");
  PK2_REQUIRE(!lm || (std::isfinite(lm_weight) && std::isfinite(insertion_bonus)), "ctc beam search: non-finite LM weight or bonus");
  int32_t Tmax = 0;
  for (int32_t n = 0; n < num_utts; ++n) {
    PK2_REQUIRE(lengths[n] >= 0 && lengths[n] <= T, "ctc beam search: utterance %d has %d frames, the tensor %d", n, lengths[n], T);
    Tmax = std::max(Tmax, lengths[n]);
  }
  const size_t need = pk2_ctc_beam_workspace_bytes(num_utts, T, num_classes, beam, top_tokens);
  PK2_REQUIRE(workspace_bytes >= need, "ctc beam search: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  PK2_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "ctc beam search: the workspace must be 256-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  CbParams p;
  memset(&p, 0, sizeof(p));
  p.lengths = lengths_dev; p.x = logits; p.ss = seq_stride; p.fs = frame_stride;
  p.Tpad = T; p.P = num_classes; p.blank = blank; p.B = beam; p.K = std::min(top_tokens, num_classes - 1);
  if (lm) {
    p.lm = ngram_trie(*lm); p.lm_start = lm->start; p.lm_eos = lm->eos; p.has_lm = 1; p.use_eos = lm_eos ? 1 : 0;
    p.lm_ids = lm_ids; p.lm_weight = lm_weight; p.bonus = insertion_bonus;
  }
  p.rows = static_cast<float*>(workspace);
  p.bp = reinterpret_cast<int2*>(static_cast<char*>(workspace) + cb_rows_bytes(num_utts, T, p.K));
  p.out_tokens = out_tokens; p.out_lens = out_lens; p.out_scores = out_scores; p.out_status = out_status;
  if (Tmax > 0)
    hipLaunchKernelGGL(ctcb_rows, dim3(std::min(256, (Tmax + 3) / 4), num_utts), dim3(256), 0, stream, lengths_dev, logits, seq_stride,
                       frame_stride, T, num_classes, blank, p.K, p.rows);
  const size_t lds = cb_lds(p.B, p.K).bytes;
  if (lds > 64 * 1024)
    PK2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ctcb_search), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ctcb_search, dim3(num_utts), dim3(kThreads), lds, stream, p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
