// Forced-alignment Viterbi on gfx950: one workgroup per utterance aligns it on its training graph (csrc/align_graph.hip)
// against log-likelihoods that stay where the model wrote them.  Replaces the reference's per-utterance host Viterbi
// after a device-to-host copy (bin/train_se2.py:263-266: kaldi.alignment.MappedAligner.align).
//
// Arithmetic (f32, each operation rounded; tests/test_gpu_align.py emulates it bit for bit):
//   ac          = (-acoustic_scale) * loglike[t, pdf]
//   cand(arc)   = (prev[src] + w) + ac             prev[-1] = 0 at t = 0 and +inf after
//   cost_t[s]   = min over the in-arcs of s in stored order, strict <, so ties go to the lowest arc
//   pruning     prev[src] counts as +inf when prev[src] > best_{t-1} + beam, best = min over all states (fmin)
//   end         total[s] = pruned cost_{T-1}[s] + final[s]; the lowest s with the least total wins;
//               none finite -> status 1 (no final state within the beam)
//   backtrace   from that state; graph = ((w_0 + w_1) + ... + w_{T-1}) + final, acoustic = ac_0 + ... + ac_{T-1}
// The frame loop is a chain of dependent steps with one barrier each: the wave minima of frame t are published in LDS
// next to the costs (double-buffered), and every thread forms best_t itself at the start of frame t + 1.  The two
// log-likelihoods a state needs at frame t + 1 (forward and self-loop pdf) are gathered before frame t's barrier.
// Costs, in-arc offsets and arcs sit in LDS when the graph fits (12 B per state + 8 B per arc); otherwise (or with
// PK2_ALIGN_LDS=0) costs live in the workspace and the graph is read from the packed buffer.
#include <cmath>
#include <cstdlib>

#include "align_internal.h"
#include "common.h"

struct pk2_align_graphs;

namespace pk2 {
void align_graphs_limits(const pk2_align_graphs* G, int32_t* num_utts, int32_t* max_states, int32_t* max_pdf, int32_t* max_arcs,
                         size_t* ws_bytes, const int32_t** packed);
}

namespace {

constexpr int kThreads = pk2::kAlignThreads;
constexpr int kWaves = kThreads / 64;
constexpr size_t kLdsLimit = 160 * 1024 - 1024;   // dynamic LDS; the static arrays below take < 1 KiB

__device__ __forceinline__ void block_sync(bool global) {
  if (global) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  } else {
    __syncthreads();
  }
}

template <int SPT, bool kLds>
__global__ __launch_bounds__(kThreads) void align_viterbi_kernel(const int32_t* __restrict__ pk, const float* __restrict__ ll,
                                                                 int64_t seq_stride, int64_t frame_stride, int32_t Tmax,
                                                                 float acoustic_scale, float beam, int32_t* __restrict__ ali,
                                                                 float* __restrict__ costs, int32_t* __restrict__ status,
                                                                 char* __restrict__ ws) {
  extern __shared__ __align__(16) char smem[];
  __shared__ float wmin[2][kWaves];
  __shared__ float red_v[kWaves];
  __shared__ int32_t red_s[kWaves];
  const float INF = __builtin_inff();
  const int n = blockIdx.x, tx = threadIdx.x, lane = tx & 63, wave = tx >> 6;
  const pk2::AlignDesc d = reinterpret_cast<const pk2::AlignDesc*>(pk)[n];
  int32_t* out = ali + (int64_t)n * Tmax;
  const int S = d.S, A = d.A, T = d.T;
  if (S == 0) {     // compiled without a path (status 2) or not at all (3)
    for (int t = tx; t < Tmax; t += kThreads) out[t] = 0;
    if (tx == 0) {
      costs[3 * n] = costs[3 * n + 1] = costs[3 * n + 2] = INF;
      status[n] = d.status;
    }
    return;
  }
  const int32_t* g_off = pk + d.in_off;
  const int32_t* g_arcx = pk + d.arcx;
  const float* g_w = reinterpret_cast<const float*>(pk + d.w);
  const float* g_fin = reinterpret_cast<const float*>(pk + d.fin);
  float* scr = reinterpret_cast<float*>(ws + d.scr);
  float *c0, *c1;
  const int32_t *off, *arcx;
  const float* w;
  if (kLds) {
    c0 = reinterpret_cast<float*>(smem);
    c1 = c0 + S;
    int32_t* l_off = reinterpret_cast<int32_t*>(c1 + S);
    int32_t* l_arcx = l_off + S + 1;
    float* l_w = reinterpret_cast<float*>(l_arcx + A);
    for (int i = tx; i <= S; i += kThreads) l_off[i] = g_off[i];
    for (int i = tx; i < A; i += kThreads) { l_arcx[i] = g_arcx[i]; l_w[i] = g_w[i]; }
    off = l_off; arcx = l_arcx; w = l_w;
  } else {
    c0 = scr;
    c1 = scr + S;
    off = g_off; arcx = g_arcx; w = g_w;
  }
  // frame 0 reads c1 as "previous": +inf everywhere
  for (int i = tx; i < S; i += kThreads) c1[i] = INF;
  const float nscale = -acoustic_scale;
  const float* row = ll + (int64_t)n * seq_stride;
  int32_t ob[SPT], oe[SPT], fp[SPT], lp[SPT];
  float af[SPT], al[SPT];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tx + j * kThreads;
    ob[j] = oe[j] = 0; fp[j] = lp[j] = 0; af[j] = al[j] = 0.f;
    if (s < S) {
      fp[j] = pk[d.fpdf + s]; lp[j] = pk[d.lpdf + s];
      af[j] = nscale * row[fp[j]];
      al[j] = nscale * row[lp[j]];
    }
  }
  block_sync(!kLds);
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tx + j * kThreads;
    if (s < S) { ob[j] = off[s]; oe[j] = off[s + 1]; }
  }
  uint32_t* bp = reinterpret_cast<uint32_t*>(ws + d.bp);
  for (int t = 0; t < T; ++t) {
    float thr = INF;
    if (t > 0) {
      float b = wmin[(t - 1) & 1][0];
#pragma unroll
      for (int q = 1; q < kWaves; ++q) b = fminf(b, wmin[(t - 1) & 1][q]);
      thr = b + beam;
    }
    const float start_v = t == 0 ? 0.f : INF;
    const float* prev = (t & 1) ? c0 : c1;
    float* cur = (t & 1) ? c1 : c0;
    uint32_t* bpt = bp + (int64_t)t * S;
    float mymin = INF;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tx + j * kThreads;
      if (s < S) {
        float best = INF;
        uint32_t arg = 0;
        for (int k = ob[j]; k < oe[j]; ++k) {
          const int32_t x = arcx[k];
          const int32_t src = (x >> 1) - 1;
          float v = start_v;
          if (src >= 0) {
            v = prev[src];
            v = v > thr ? INF : v;
          }
          const float cand = (v + w[k]) + ((x & 1) ? al[j] : af[j]);
          if (cand < best) { best = cand; arg = ((uint32_t)(src + 1) << 16) | (uint32_t)(k - ob[j]); }
        }
        cur[s] = best;
        bpt[s] = arg;
        mymin = fminf(mymin, best);
      }
    }
    if (t + 1 < T) {     // gather frame t + 1 before the barrier
      row += frame_stride;
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        if (tx + j * kThreads < S) { af[j] = nscale * row[fp[j]]; al[j] = nscale * row[lp[j]]; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mymin = fminf(mymin, __shfl_xor(mymin, o));
    if (lane == 0) wmin[t & 1][wave] = mymin;
    block_sync(!kLds);
  }
  // ---- the best final state
  float thr = wmin[(T - 1) & 1][0];
  for (int q = 1; q < kWaves; ++q) thr = fminf(thr, wmin[(T - 1) & 1][q]);
  thr = thr + beam;
  const float* last = ((T - 1) & 1) ? c1 : c0;
  float bv = INF;
  int32_t bs = INT32_MAX;
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tx + j * kThreads;
    if (s < S) {
      float v = last[s];
      v = v > thr ? INF : v;
      const float tot = v + g_fin[s];
      if (tot < bv) { bv = tot; bs = s; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bv, o);
    const int32_t s2 = __shfl_xor(bs, o);
    if (v2 < bv || (v2 == bv && s2 < bs)) { bv = v2; bs = s2; }
  }
  if (lane == 0) { red_v[wave] = bv; red_s[wave] = bs; }
  __syncthreads();
  bv = red_v[0]; bs = red_s[0];
  for (int q = 1; q < kWaves; ++q)
    if (red_v[q] < bv || (red_v[q] == bv && red_s[q] < bs)) { bv = red_v[q]; bs = red_s[q]; }
  if (!(bv < INF)) {
    for (int t = tx; t < Tmax; t += kThreads) out[t] = 0;
    if (tx == 0) {
      costs[3 * n] = costs[3 * n + 1] = costs[3 * n + 2] = INF;
      status[n] = 1;
    }
    return;
  }
  // ---- backtrace: one lane follows the chain (one dependent load per frame), the arc of frame t goes to out[t]
  if (tx == 0) {
    int32_t s = bs;
    for (int t = T - 1; t >= 0; --t) {
      const uint32_t e = bp[(int64_t)t * S + s];
      out[t] = g_off[s] + (int32_t)(e & 0xffffu);
      s = (int32_t)(e >> 16) - 1;
      if (s < 0 && t > 0) {      // cannot happen on a consistent table; never read outside it
        for (int u = 0; u < t; ++u) out[u] = out[t];
        break;
      }
    }
  }
  block_sync(true);
  float* sw = scr + 2 * S;
  float* sa = sw + T;
  const int32_t* g_tid = pk + d.tid;
  const int32_t* g_pdf = pk + d.pdf;
  const float* row0 = ll + (int64_t)n * seq_stride;
  for (int t = tx; t < Tmax; t += kThreads) {
    if (t < T) {
      const int32_t k = out[t];
      sw[t] = g_w[k];
      sa[t] = nscale * row0[(int64_t)t * frame_stride + g_pdf[k]];
      out[t] = g_tid[k];
    } else {
      out[t] = 0;
    }
  }
  block_sync(true);
  if (tx == 0) {
    float gsum = 0.f, asum = 0.f;
    for (int t = 0; t < T; ++t) { gsum = gsum + sw[t]; asum = asum + sa[t]; }
    costs[3 * n] = bv;
    costs[3 * n + 1] = gsum + g_fin[bs];
    costs[3 * n + 2] = asum;
    status[n] = 0;
  }
}

template <int SPT, bool kLds>
int launch(const int32_t* pk, int32_t N, const float* ll, int64_t ss, int64_t fs, int32_t Tmax, float ascale, float beam,
           int32_t* ali, float* costs, int32_t* status, char* ws, size_t lds, hipStream_t stream) {
  auto fn = &align_viterbi_kernel<SPT, kLds>;
  if (kLds && lds > 64 * 1024)
    PK2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fn, dim3(N), dim3(kThreads), kLds ? lds : 0, stream, pk, ll, ss, fs, Tmax, ascale, beam, ali, costs,
                     status, ws);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

template <bool kLds>
int dispatch(int spt, const int32_t* pk, int32_t N, const float* ll, int64_t ss, int64_t fs, int32_t Tmax, float ascale,
             float beam, int32_t* ali, float* costs, int32_t* status, char* ws, size_t lds, hipStream_t stream) {
  switch (spt) {
    case 1: return launch<1, kLds>(pk, N, ll, ss, fs, Tmax, ascale, beam, ali, costs, status, ws, lds, stream);
    case 2: return launch<2, kLds>(pk, N, ll, ss, fs, Tmax, ascale, beam, ali, costs, status, ws, lds, stream);
    case 4: return launch<4, kLds>(pk, N, ll, ss, fs, Tmax, ascale, beam, ali, costs, status, ws, lds, stream);
    case 8: return launch<8, kLds>(pk, N, ll, ss, fs, Tmax, ascale, beam, ali, costs, status, ws, lds, stream);
    case 16: return launch<16, kLds>(pk, N, ll, ss, fs, Tmax, ascale, beam, ali, costs, status, ws, lds, stream);
    default: return launch<32, kLds>(pk, N, ll, ss, fs, Tmax, ascale, beam, ali, costs, status, ws, lds, stream);
  }
}

}  // namespace

extern "C" {

int pk2_align_use_lds(const pk2_align_graphs* G) {
  if (!G) return 0;
  int32_t N, S, P, A;
  size_t wsb;
  const int32_t* packed;
  pk2::align_graphs_limits(G, &N, &S, &P, &A, &wsb, &packed);
  const char* e = getenv("PK2_ALIGN_LDS");
  if (e && e[0] == '0') return 0;
  return pk2::align_up(12 * (size_t)S + 4 + 8 * (size_t)A, 16) <= kLdsLimit ? 1 : 0;
}

int pk2_align_viterbi(const pk2_align_graphs* G, const int32_t* packed_dev, const float* loglikes, int64_t seq_stride,
                      int64_t frame_stride, int32_t num_pdfs, int32_t Tmax, float acoustic_scale, float beam,
                      int32_t* alignment, float* costs, int32_t* status, void* workspace, size_t workspace_bytes,
                      void* stream) {
  PK2_REQUIRE(G && packed_dev && loglikes && alignment && costs && status && workspace, "pk2_align_viterbi: null argument");
  int32_t N, S, P, A;
  size_t wsb;
  const int32_t* packed;
  pk2::align_graphs_limits(G, &N, &S, &P, &A, &wsb, &packed);
  PK2_REQUIRE(P < num_pdfs, "pk2_align_viterbi: the graphs use pdf %d, the log-likelihoods have %d columns", P, num_pdfs);
  PK2_REQUIRE(workspace_bytes >= wsb, "pk2_align_viterbi: workspace of %zu bytes, %zu needed", workspace_bytes, wsb);
  PK2_REQUIRE(S <= pk2::kAlignMaxStates, "pk2_align_viterbi: %d states", S);
  PK2_REQUIRE(frame_stride >= num_pdfs && seq_stride >= 0, "pk2_align_viterbi: bad strides");
  for (int32_t n = 0; n < N; ++n)
    PK2_REQUIRE(reinterpret_cast<const pk2::AlignDesc*>(packed)[n].T <= Tmax, "pk2_align_viterbi: utterance %d is longer than Tmax = %d", n, Tmax);
  int spt = 1;
  while (spt * kThreads < S) spt *= 2;
  const size_t lds = pk2::align_up(12 * (size_t)S + 4 + 8 * (size_t)A, 16);
  auto s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  if (pk2_align_use_lds(G))
    return dispatch<true>(spt, packed_dev, N, loglikes, seq_stride, frame_stride, Tmax, acoustic_scale, beam, alignment, costs,
                          status, ws, lds, s);
  return dispatch<false>(spt, packed_dev, N, loglikes, seq_stride, frame_stride, Tmax, acoustic_scale, beam, alignment, costs,
                         status, ws, 0, s);
}

}  // extern "C"
