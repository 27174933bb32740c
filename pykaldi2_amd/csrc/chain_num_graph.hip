// Alignment-free LF-MMI numerator on gfx950: the full-sum forward-backward of every utterance over its cyclic training
// graph (transcript x L.fst x tree x H, csrc/align_graph.hip), read from the packed AlignDesc buffer the forced aligner
// uses (csrc/align_internal.h).  Kaldi's counterpart is GenericNumeratorComputation (chain-generic-numerator.cc), which
// works on the host in the log domain; here the recursions run in probability space, f32, with one scale per frame
// (DESIGN.md 7.6).
//
//   alpha_0(d) = sum_{a: dst=d, src=-1} e^{-w_a} x_0(pdf_a)        alpha_t(d) = sum_{a: dst=d} alpha_{t-1}(src_a) e^{-w_a} x_t(pdf_a)
//   beta_{T-1}(s) = e^{-fin(s)}                                    beta_t(s)  = sum_{a: src=s} e^{-w_a} x_{t+1}(pdf_a) beta_{t+1}(dst_a)
//   log p = log sum_s alpha_{T-1}(s) e^{-fin(s)}                   gamma_t(p) = sum_{a: pdf_a=p} P(arc a at frame t)
//
// Four launches on one stream, none waits on another workgroup:
//   ng_setup   the out-arc lists the beta chain needs (the packed graph holds in-arcs only) and the (state, forward |
//              self-loop) slots sorted by pdf, both by counting ranks: every result has one writer, in a fixed place.
//   ng_scores  parallel over frames: m_t = max over the utterance's pdfs, b_t(s) = exp(x_t(fpdf_s) - m_t), exp(x_t(lpdf_s) - m_t)
//              per STATE (two coalesced columns instead of a list of distinct pdfs: the chains then load them without a gather).
//   ng_chains  two workgroups per utterance: alpha from frame 0 up, beta from frame T-1 down, states over the 512
//              lanes, one barrier per frame.  What is stored at frame t carries the scales lazily: with z_t the sum of
//              the stored alpha row, a_t(d) = [sum_a a_{t-1}(src) e^{-w} b_t] / z_{t-1}, kept split by arc kind
//              (forward / self-loop) so that the posterior pass needs no graph; true alpha_t = a_t e^{m_0 + .. + m_t} z_0 .. z_{t-1}.
//              log p = sum_t m_t + sum_{t < T-1} log z_t + log sum_s a_{T-1}(s) e^{-fin(s)}, the sums in double.
//   ng_post    one workgroup per frame: q(s, kind) = a_t(s, kind) * bhat_t(s), normalised by the frame's own sum (the
//              product of the two chains' scales cancels against p, as in csrc/chain_num.h), then one thread per
//              distinct pdf adds its slots in sorted order into grad: no atomics, the result is bit-reproducible.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "align_internal.h"
#include "chain_num_graph.h"
#include "common.h"

struct pk2_align_graphs;

namespace pk2 {
void align_graphs_limits(const pk2_align_graphs* G, int32_t* num_utts, int32_t* max_states, int32_t* max_pdf, int32_t* max_arcs,
                         size_t* ws_bytes, const int32_t** packed);
}

namespace {

using pk2::AlignDesc;
constexpr int kThreads = pk2::kAlignThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kPre = 2;                           // states per thread whose next-frame factors are loaded ahead of the barrier
constexpr size_t kLdsLimit = 160 * 1024 - 1024;

// Workspace of one utterance, in floats / int32 words from its base (every array on a 64-word boundary).
struct NgLayout {
  size_t b2, mt, a2, bh, az, o_x, o_e, o_off, order, spdf, scr, words;
};
__host__ __device__ inline size_t ng_up(size_t x) { return (x + 63) / 64 * 64; }
__host__ __device__ inline NgLayout ng_layout(size_t S, size_t A, size_t T) {
  NgLayout l;
  size_t o = 0;
  l.b2 = o; o += ng_up(2 * T * S);      // f32 [T][S][2]  exp(x - m) of the forward / self-loop pdf
  l.mt = o; o += ng_up(T);              // f32 [T]        frame maxima
  l.a2 = o; o += ng_up(2 * T * S);      // f32 [T][S][2]  stored alpha, split by arc kind
  l.bh = o; o += ng_up(T * S);          // f32 [T][S]     stored beta
  l.az = o; o += ng_up(T);              // f32 [T]        z_t
  l.o_x = o; o += ng_up(A);             // i32 [A]        out-arcs sorted by (src, arc): dst << 1 | self_loop
  l.o_e = o; o += ng_up(A);             // f32 [A]        their e^{-w}
  l.o_off = o; o += ng_up(S + 1);       // i32 [S+1]      out-arcs of s: o_off[s] .. o_off[s+1]
  l.order = o; o += ng_up(2 * S);       // i32 [2S]       slots 2 s + kind sorted by (pdf, slot)
  l.spdf = o; o += ng_up(2 * S);        // i32 [2S]       their pdfs
  l.scr = o; o += ng_up(4 * S);         // f32 [2][2S]    the beta chain's working vectors when they are not in LDS
  l.words = o;
  return l;
}
// Base (in words) of utterance n: the utterances' blocks follow each other in order.
__device__ inline size_t ng_base(const AlignDesc* desc, int n) {
  size_t o = 0;
  for (int m = 0; m < n; ++m)
    if (desc[m].S > 0) o += ng_layout(desc[m].S, desc[m].A, desc[m].T).words;
  return o;
}

__device__ __forceinline__ void block_sync(bool global) {
  if (global) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  } else {
    __syncthreads();
  }
}

// ---- ng_setup: grid (blocks, N, 3).  z = 0: out-arcs; z = 1: o_off; z = 2: slots by pdf.  The rank of an item is the number
// of items with a smaller key (keys are distinct), counted against LDS tiles of the whole list.
__global__ __launch_bounds__(256) void ng_setup(const int32_t* __restrict__ pk, float* __restrict__ ws) {
  __shared__ unsigned long long tile[256];
  const int n = blockIdx.y, mode = blockIdx.z, tx = threadIdx.x;
  const AlignDesc* desc = reinterpret_cast<const AlignDesc*>(pk);
  const AlignDesc d = desc[n];
  const int S = d.S, A = d.A;
  if (S == 0) return;
  const int items = mode == 0 ? A : mode == 1 ? S + 1 : 2 * S;      // what this pass ranks
  const int others = mode == 2 ? 2 * S : A;                         // ... against what
  if ((int)blockIdx.x * 256 >= items) return;
  const NgLayout l = ng_layout(S, A, d.T);
  float* base = ws + ng_base(desc, n);
  const int32_t* arcx = pk + d.arcx;
  const int32_t* fpdf = pk + d.fpdf;
  const int32_t* lpdf = pk + d.lpdf;
  auto key_of = [&](int i) -> unsigned long long {                  // key of list element i
    if (mode == 2) return ((unsigned long long)(uint32_t)((i & 1) ? lpdf[i >> 1] : fpdf[i >> 1]) << 32) | (uint32_t)i;
    return ((unsigned long long)(uint32_t)(arcx[i] >> 1) << 32) | (uint32_t)i;      // (src + 1, arc)
  };
  const int i = blockIdx.x * 256 + tx;
  unsigned long long mine = 0;
  if (i < items) mine = mode == 1 ? ((unsigned long long)(uint32_t)(i + 1) << 32) : key_of(i);   // mode 1: arcs with src < i
  int rank = 0;
  for (int t0 = 0; t0 < others; t0 += 256) {
    __syncthreads();
    if (t0 + tx < others) tile[tx] = key_of(t0 + tx);
    __syncthreads();
    const int cnt = min(256, others - t0);
    if (i < items)
      for (int k = 0; k < cnt; ++k) rank += tile[k] < mine ? 1 : 0;
  }
  if (i >= items) return;
  if (mode == 0) {
    const int32_t* in_off = pk + d.in_off;
    int lo = 0, hi = S;                                             // the state whose in-arc list holds arc i
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (in_off[mid] <= i) lo = mid; else hi = mid;
    }
    reinterpret_cast<int32_t*>(base + l.o_x)[rank] = (lo << 1) | (arcx[i] & 1);
    (base + l.o_e)[rank] = __expf(-reinterpret_cast<const float*>(pk + d.w)[i]);
  } else if (mode == 1) {
    reinterpret_cast<int32_t*>(base + l.o_off)[i] = rank;
  } else {
    reinterpret_cast<int32_t*>(base + l.order)[rank] = i;
    reinterpret_cast<int32_t*>(base + l.spdf)[rank] = (i & 1) ? lpdf[i >> 1] : fpdf[i >> 1];
  }
}

// ---- ng_scores: a wave per frame.
__global__ __launch_bounds__(256) void ng_scores(const int32_t* __restrict__ pk, const float* __restrict__ logits, int64_t seq_stride,
                                                 int64_t frame_stride, float* __restrict__ ws) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const AlignDesc* desc = reinterpret_cast<const AlignDesc*>(pk);
  const AlignDesc d = desc[n];
  const int S = d.S, T = d.T;
  if (S == 0) return;
  const NgLayout l = ng_layout(S, d.A, T);
  float* base = ws + ng_base(desc, n);
  const int32_t* fpdf = pk + d.fpdf;
  const int32_t* lpdf = pk + d.lpdf;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  for (int t = wave; t < T; t += nwaves) {
    const float* row = logits + (int64_t)n * seq_stride + (int64_t)t * frame_stride;
    float m = -INFINITY;
    for (int s = lane; s < S; s += 64) m = fmaxf(m, fmaxf(row[fpdf[s]], row[lpdf[s]]));
    m = pk2::wave_max(m);
    float2* b = reinterpret_cast<float2*>(base + l.b2) + (size_t)t * S;
    for (int s = lane; s < S; s += 64) b[s] = make_float2(__expf(row[fpdf[s]] - m), __expf(row[lpdf[s]] - m));
    if (lane == 0) (base + l.mt)[t] = m;
  }
}

// ---- ng_chains: grid (2, N).  blockIdx.x = 0: alpha and log p; 1: beta.
template <bool kLds>
__global__ __launch_bounds__(kThreads) void ng_chains(const int32_t* __restrict__ pk, float* __restrict__ ws, float* __restrict__ logprob,
                                                      int32_t* __restrict__ status) {
  extern __shared__ __align__(16) char smem[];
  __shared__ float wsum[2][kWaves];
  __shared__ double dred[kWaves];
  const int n = blockIdx.y, tx = threadIdx.x, lane = tx & 63, wave = tx >> 6;
  const bool fwd = blockIdx.x == 0;
  const AlignDesc* desc = reinterpret_cast<const AlignDesc*>(pk);
  const AlignDesc d = desc[n];
  const int S = d.S, A = d.A, T = d.T;
  if (S == 0) {
    if (fwd && tx == 0) { logprob[n] = 0.f; status[n] = d.status; }
    return;
  }
  const NgLayout l = ng_layout(S, A, T);
  float* base = ws + ng_base(desc, n);
  const float2* b2 = reinterpret_cast<const float2*>(base + l.b2);
  auto frame_sum = [&](int t) {
    float z = wsum[t & 1][0];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) z += wsum[t & 1][q];
    return z;
  };
  auto publish = [&](int t, float v) {
    v = pk2::wave_sum(v);
    if (lane == 0) wsum[t & 1][wave] = v;
  };
  if (fwd) {
    // in-arcs: offsets, arcx and e^{-w}; the previous row (kind-summed) in two LDS vectors, or read back from a2
    const int32_t* g_off = pk + d.in_off;
    const int32_t* g_arcx = pk + d.arcx;
    const float* g_w = reinterpret_cast<const float*>(pk + d.w);
    float2* a2 = reinterpret_cast<float2*>(base + l.a2);
    float* az = base + l.az;
    float *c0 = nullptr, *c1 = nullptr, *l_e = nullptr;
    const int32_t *off = g_off, *arcx = g_arcx;
    if (kLds) {
      c0 = reinterpret_cast<float*>(smem);
      c1 = c0 + S;
      int32_t* l_off = reinterpret_cast<int32_t*>(c1 + S);
      int32_t* l_arcx = l_off + S + 1;
      l_e = reinterpret_cast<float*>(l_arcx + A);
      for (int i = tx; i <= S; i += kThreads) l_off[i] = g_off[i];
      for (int i = tx; i < A; i += kThreads) { l_arcx[i] = g_arcx[i]; l_e[i] = __expf(-g_w[i]); }
      off = l_off; arcx = l_arcx;
    }
    float2 pre[kPre];
#pragma unroll
    for (int j = 0; j < kPre; ++j) {
      const int s = tx + j * kThreads;
      pre[j] = s < S ? b2[s] : make_float2(0.f, 0.f);
    }
    block_sync(!kLds);
    for (int t = 0; t < T; ++t) {
      float inv = 1.f;
      if (t > 0) {
        const float z = frame_sum(t - 1);
        inv = 1.f / z;
        if (tx == 0) az[t - 1] = z;
      }
      const float* prev = (t & 1) ? c0 : c1;
      float* cur = (t & 1) ? c1 : c0;
      const float2* prow = a2 + (size_t)(t - 1) * S;      // (read only when t > 0)
      float2* arow = a2 + (size_t)t * S;
      const float2* brow = b2 + (size_t)t * S;
      float mysum = 0.f;
      for (int s = tx, j = 0; s < S; s += kThreads, ++j) {
        float accf = 0.f, accl = 0.f;
        const int ke = off[s + 1];
        for (int k = off[s]; k < ke; ++k) {
          const int32_t x = arcx[k];
          const int32_t src = (x >> 1) - 1;
          float v;
          if (src < 0) v = t == 0 ? 1.f : 0.f;
          else if (t == 0) v = 0.f;
          else if (kLds) v = prev[src];
          else { const float2 p = prow[src]; v = p.x + p.y; }
          const float e = kLds ? l_e[k] : __expf(-g_w[k]);
          if (x & 1) accl += v * e; else accf += v * e;
        }
        float2 b;
        if (j < kPre) b = j == 0 ? pre[0] : pre[1]; else b = brow[s];
        const float af = accf * b.x * inv, al = accl * b.y * inv;
        arow[s] = make_float2(af, al);
        if (kLds) cur[s] = af + al;
        mysum += af + al;
      }
      if (t + 1 < T) {
        const float2* nrow = b2 + (size_t)(t + 1) * S;
#pragma unroll
        for (int j = 0; j < kPre; ++j) {
          const int s = tx + j * kThreads;
          if (s < S) pre[j] = nrow[s];
        }
      }
      publish(t, mysum);
      block_sync(!kLds);
    }
    // log p: frame maxima, log of the frame sums (all but the last), the final states on the last row
    const float* g_fin = reinterpret_cast<const float*>(pk + d.fin);
    if (tx == 0) az[T - 1] = frame_sum(T - 1);
    block_sync(true);
    const float* mt = base + l.mt;
    double acc = 0.0;
    for (int t = tx; t < T; t += kThreads) acc += (double)mt[t] + (t + 1 < T ? log((double)az[t]) : 0.0);
    acc = pk2::wave_sum_d(acc);
    float zf = 0.f;
    const float2* last = a2 + (size_t)(T - 1) * S;
    for (int s = tx; s < S; s += kThreads) {
      const float f = g_fin[s];
      if (f < INFINITY) { const float2 p = last[s]; zf += (p.x + p.y) * __expf(-f); }
    }
    publish(T, zf);
    if (lane == 0) dred[wave] = acc;
    __syncthreads();
    if (tx == 0) {
      double tot = 0.0;
      for (int q = 0; q < kWaves; ++q) tot += dred[q];
      logprob[n] = (float)(tot + log((double)frame_sum(T)));
      status[n] = 0;
    }
  } else {
    // out-arcs from the workspace (ng_setup); u_t(2 d + kind) = bhat_t(d) * b_t(d, kind) is what frame t - 1 gathers
    const int32_t* g_off = reinterpret_cast<const int32_t*>(base + l.o_off);
    const int32_t* g_ox = reinterpret_cast<const int32_t*>(base + l.o_x);
    const float* g_oe = base + l.o_e;
    const float* g_fin = reinterpret_cast<const float*>(pk + d.fin);
    float* bh = base + l.bh;
    float *u0, *u1;
    const int32_t *off = g_off, *ox = g_ox;
    const float* oe = g_oe;
    if (kLds) {
      u0 = reinterpret_cast<float*>(smem);
      u1 = u0 + 2 * S;
      int32_t* l_off = reinterpret_cast<int32_t*>(u1 + 2 * S);
      int32_t* l_ox = l_off + S + 1;
      float* l_oe = reinterpret_cast<float*>(l_ox + A);
      for (int i = tx; i <= S; i += kThreads) l_off[i] = g_off[i];
      for (int i = tx; i < A; i += kThreads) { l_ox[i] = g_ox[i]; l_oe[i] = g_oe[i]; }
      off = l_off; ox = l_ox; oe = l_oe;
    } else {
      u0 = base + l.scr;
      u1 = u0 + 2 * S;
    }
    float2 pre[kPre];
#pragma unroll
    for (int j = 0; j < kPre; ++j) {
      const int s = tx + j * kThreads;
      pre[j] = s < S ? b2[(size_t)(T - 1) * S + s] : make_float2(0.f, 0.f);
    }
    block_sync(!kLds);
    for (int t = T - 1; t >= 0; --t) {
      const float inv = t == T - 1 ? 1.f : 1.f / frame_sum(t + 1);
      const float* prev = (t & 1) ? u0 : u1;
      float* cur = (t & 1) ? u1 : u0;
      float* hrow = bh + (size_t)t * S;
      const float2* brow = b2 + (size_t)t * S;
      float mysum = 0.f;
      for (int s = tx, j = 0; s < S; s += kThreads, ++j) {
        float h;
        if (t == T - 1) {
          const float f = g_fin[s];
          h = f < INFINITY ? __expf(-f) : 0.f;
        } else {
          float acc = 0.f;
          const int ke = off[s + 1];
          for (int k = off[s]; k < ke; ++k) acc += oe[k] * prev[ox[k]];
          h = acc * inv;
        }
        float2 b;
        if (j < kPre) b = j == 0 ? pre[0] : pre[1]; else b = brow[s];
        hrow[s] = h;
        cur[2 * s] = h * b.x;
        cur[2 * s + 1] = h * b.y;
        mysum += h;
      }
      if (t > 0) {
        const float2* nrow = b2 + (size_t)(t - 1) * S;
#pragma unroll
        for (int j = 0; j < kPre; ++j) {
          const int s = tx + j * kThreads;
          if (s < S) pre[j] = nrow[s];
        }
      }
      publish(t, mysum);
      block_sync(!kLds);
    }
  }
}

// ---- ng_post: grid (Tmax, N), 256 threads, 2 S floats of LDS.
__global__ __launch_bounds__(256) void ng_post(const int32_t* __restrict__ pk, const float* __restrict__ ws, float scale,
                                               float* __restrict__ grad, int64_t gss, int64_t gfs) {
  extern __shared__ __align__(16) char smem[];
  __shared__ float red[4];
  float* q = reinterpret_cast<float*>(smem);
  const int n = blockIdx.y, t = blockIdx.x, tx = threadIdx.x;
  const AlignDesc* desc = reinterpret_cast<const AlignDesc*>(pk);
  const AlignDesc d = desc[n];
  const int S = d.S;
  if (S == 0 || t >= d.T) return;
  const NgLayout l = ng_layout(S, d.A, d.T);
  const float* base = ws + ng_base(desc, n);
  const float2* arow = reinterpret_cast<const float2*>(base + l.a2) + (size_t)t * S;
  const float* hrow = base + l.bh + (size_t)t * S;
  float mysum = 0.f;
  for (int s = tx; s < S; s += 256) {
    const float2 a = arow[s];
    const float h = hrow[s];
    const float qf = a.x * h, ql = a.y * h;
    q[2 * s] = qf;
    q[2 * s + 1] = ql;
    mysum += qf + ql;
  }
  mysum = pk2::wave_sum(mysum);
  if ((tx & 63) == 0) red[tx >> 6] = mysum;
  __syncthreads();
  const float f = scale / ((red[0] + red[1]) + (red[2] + red[3]));
  const int32_t* order = reinterpret_cast<const int32_t*>(base + l.order);
  const int32_t* spdf = reinterpret_cast<const int32_t*>(base + l.spdf);
  float* grow = grad + (int64_t)n * gss + (int64_t)t * gfs;
  for (int r = tx; r < 2 * S; r += 256) {
    const int32_t p = spdf[r];
    if (r > 0 && spdf[r - 1] == p) continue;      // the first slot of a pdf adds the whole group, in sorted order
    float acc = 0.f;
    for (int k = r; k < 2 * S && spdf[k] == p; ++k) acc += q[order[k]];
    grow[p] += acc * f;
  }
}

struct Limits {
  int32_t N, S, P, A;
  const AlignDesc* desc;
  size_t lds;
};
Limits limits_of(const pk2_align_graphs* G) {
  Limits L;
  size_t wsb;
  const int32_t* packed;
  pk2::align_graphs_limits(G, &L.N, &L.S, &L.P, &L.A, &wsb, &packed);
  L.desc = reinterpret_cast<const AlignDesc*>(packed);
  L.lds = pk2::align_up(20 * (size_t)L.S + 4 + 8 * (size_t)L.A, 16);     // the beta chain's need; alpha's is 12 S + 4 + 8 A
  for (int32_t n = 0; n < L.N; ++n) {      // the pre-pass reads fpdf / lpdf of every state
    const AlignDesc& d = L.desc[n];
    for (int32_t s = 0; s < d.S; ++s) L.P = std::max(L.P, std::max(packed[d.fpdf + s], packed[d.lpdf + s]));
  }
  return L;
}

}  // namespace

namespace pk2 {

size_t num_graph_workspace(const pk2_align_graphs* G) {
  const Limits L = limits_of(G);
  size_t words = 0;
  for (int32_t n = 0; n < L.N; ++n)
    if (L.desc[n].S > 0) words += ng_layout(L.desc[n].S, L.desc[n].A, L.desc[n].T).words;
  return align_up(words * 4 + 256, 256);
}

int num_graph_compute(const pk2_align_graphs* G, const int32_t* packed_dev, const float* logits, int64_t seq_stride,
                      int64_t frame_stride, int32_t num_pdfs, float scale, float* grad, int64_t gss, int64_t gfs, float* logprob,
                      int32_t* status, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const Limits L = limits_of(G);
  PK2_REQUIRE(L.P < num_pdfs, "num_graph: the graphs use pdf %d, the network output has %d columns", L.P, num_pdfs);
  PK2_REQUIRE(frame_stride >= num_pdfs && gfs >= num_pdfs && seq_stride >= 0 && gss >= 0, "num_graph: bad strides");
  const size_t need = num_graph_workspace(G);
  PK2_REQUIRE(workspace_bytes >= need, "num_graph: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  PK2_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "num_graph: the workspace must be 256-byte aligned");
  PK2_REQUIRE(L.S <= kAlignMaxStates, "num_graph: %d states", L.S);
  int32_t Tmax = 0, items = 0;
  for (int32_t n = 0; n < L.N; ++n)
    if (L.desc[n].S > 0) {
      Tmax = std::max(Tmax, L.desc[n].T);
      items = std::max(items, std::max(L.desc[n].A, 2 * L.desc[n].S));
    }
  if (Tmax == 0) {      // nothing compiled: only the statuses
    hipLaunchKernelGGL(ng_chains<false>, dim3(1, L.N), dim3(kThreads), 0, stream, packed_dev, static_cast<float*>(workspace), logprob, status);
    PK2_LAUNCH_CHECK();
    return PK2_OK;
  }
  float* ws = static_cast<float*>(workspace);
  hipLaunchKernelGGL(ng_setup, dim3((items + 255) / 256, L.N, 3), dim3(256), 0, stream, packed_dev, ws);
  hipLaunchKernelGGL(ng_scores, dim3(std::max(1, std::min(64, (Tmax + 3) / 4)), L.N), dim3(256), 0, stream, packed_dev, logits,
                     seq_stride, frame_stride, ws);
  if (num_graph_use_lds(G)) {
    auto fn = &ng_chains<true>;
    if (L.lds > 64 * 1024)
      PK2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    hipLaunchKernelGGL(fn, dim3(2, L.N), dim3(kThreads), L.lds, stream, packed_dev, ws, logprob, status);
  } else {
    hipLaunchKernelGGL(ng_chains<false>, dim3(2, L.N), dim3(kThreads), 0, stream, packed_dev, ws, logprob, status);
  }
  const size_t post_lds = align_up(8 * (size_t)L.S, 16);
  if (post_lds > 64 * 1024)
    PK2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ng_post), hipFuncAttributeMaxDynamicSharedMemorySize, (int)post_lds));
  hipLaunchKernelGGL(ng_post, dim3(Tmax, L.N), dim3(256), post_lds, stream, packed_dev, ws, scale, grad, gss, gfs);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

int num_graph_use_lds(const pk2_align_graphs* G) {
  const char* e = getenv("PK2_NUM_GRAPH_LDS");
  if (e && e[0] == '0') return 0;
  return limits_of(G).lds <= kLdsLimit ? 1 : 0;
}

}  // namespace pk2

extern "C" {

size_t pk2_num_graph_workspace_bytes(const pk2_align_graphs* G) { return G ? pk2::num_graph_workspace(G) : 0; }

int pk2_num_graph_use_lds(const pk2_align_graphs* G) { return G ? pk2::num_graph_use_lds(G) : 0; }

int pk2_num_graph_fwd_bwd(const pk2_align_graphs* G, const int32_t* packed_dev, const float* logits, int64_t seq_stride,
                          int64_t frame_stride, int32_t num_pdfs, int32_t Tmax, float scale, float* grad, int64_t grad_seq_stride,
                          int64_t grad_frame_stride, float* logprob, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream) {
  PK2_REQUIRE(G && packed_dev && logits && grad && logprob && status && workspace, "pk2_num_graph_fwd_bwd: null argument");
  const Limits L = limits_of(G);
  for (int32_t n = 0; n < L.N; ++n)
    PK2_REQUIRE(L.desc[n].T <= Tmax, "pk2_num_graph_fwd_bwd: utterance %d is longer than Tmax = %d", n, Tmax);
  return pk2::num_graph_compute(G, packed_dev, logits, seq_stride, frame_stride, num_pdfs, scale, grad, grad_seq_stride,
                                grad_frame_stride, logprob, status, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
